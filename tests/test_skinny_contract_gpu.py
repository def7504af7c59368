"""cara_skinny_xu(_r), cara_tskinny_partial / partial2 / partial2_r with cara_tskinny_reduce / reduce_many, cara_tskinny_xtg,
cara_gemm_tn_f32 and cara_linear_fwd / cara_linear_bwd as stand-alone launches on the device, in both operand builds, held to the
derived bounds of oracle/skinny_model.py (proven attainable on the host by tests/test_skinny_model.py, whose cases, inputs and
restatements are shared here) at the shapes where the launch branches turn.  Every output buffer sits between GUARD sentinel words
and starts as NaN; the padding of the inputs (the columns between K and ldx, the rows of X behind row M - 1, the columns of Gt behind
roundup32(M)) holds NaN, so that a read of it shows; 16-bit outputs are under the interval rule and the cap of tests/tolerances.py
(SKINNY_CAPS), fp32 outputs under hold_f32 and the aggregate rule against the host's other-order restatement; figures are printed
(-s) before they are asserted.  Refusals return non-zero and write nothing.  docs/findings/skinny_contract.md holds the tables."""
import ctypes as C

import pytest
import torch

from oracle import gemm_model as G
from oracle import skinny_model as K
from tests import skinny_common as S
from tests import tolerances as T
from tests.test_kernels_gpu import DEV, L
from tests.test_small_kernels_gpu import GUARD, is_sentinel, sentinel

pytestmark = pytest.mark.gpu

OPERANDS = ["bf16", "fp16"]
NAN = float("nan")
SZ = C.c_size_t


def _buf(shape, dtype):
    """a NaN-filled tensor of `shape` between GUARD sentinel words on both sides -> (whole allocation, the tensor)"""
    n = 1
    for s in shape:
        n *= s
    full = sentinel((GUARD + n + GUARD,), dtype)
    full[GUARD:GUARD + n] = NAN
    return full, full[GUARD:GUARD + n].view(*shape)


def _intact(*pairs):
    return all(is_sentinel(full[:GUARD]) and is_sentinel(full[GUARD + live.numel():]) for full, live in pairs)


def _all_nan(*pairs):
    return all(bool(torch.isnan(live).all()) for _, live in pairs)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _p(t):
    return L().ptr(t)


def _st():
    return L().stream()


def _rows(X, M, Kc, dt, ld=None, behind=NAN, extra=8):
    """X [M, K] on the host -> a device allocation [M + extra, ld] whose padding columns and rows behind M - 1 hold `behind`"""
    ld = ld or Kc
    buf = torch.full((M + extra, ld), behind, dtype=dt, device=DEV)
    buf[:M, :Kc] = X[:M, :Kc].to(DEV)
    return buf


def _panels(X, M, Kc, dt, P=None, behind=NAN):
    """the K-panel-major image [K / 32][P rows][32] of X [M, K], rows M .. P - 1 of every panel `behind`"""
    P = P or M
    buf = torch.full((Kc // 32, P, 32), behind, dtype=dt, device=DEV)
    buf[:, :M] = X[:M, :Kc].to(DEV).view(M, Kc // 32, 32).permute(1, 0, 2)
    return buf


# --- cara_skinny_xu(_r) ---------------------------------------------------------------------------------------------------------
def _xu_call(lib, Xd, ldx, Utd, M, Kc, Rp, rank, dt, ldt=None, with_tt=True, plain=False, prefill=None):
    ldt = ldt if ldt is not None else K.roundup32(M)
    Tb, Ttb = _buf((M, Rp), dt), _buf((Rp, ldt), dt)
    if plain:
        rc = lib.cara_skinny_xu(_p(Xd), ldx, _p(Utd), _p(Tb[1]), _p(Ttb[1]) if with_tt else None, ldt, M, Kc, Rp, _st())
    else:
        rc = lib.cara_skinny_xu_r(_p(Xd), ldx, _p(Utd), _p(Tb[1]), _p(Ttb[1]) if with_tt else None, ldt, M, Kc, Rp, rank, _st())
    torch.cuda.synchronize()
    return rc, Tb, Ttb


def _hold_xu(tag, model, Tb, Ttb, M, dt, name="T"):
    """T inside its bound and cap, Tt[:, :M] its transpose bit for bit, the pad zero in bits, the rest of Tt untouched, guards intact"""
    T_, Tt = Tb[1].cpu(), Ttb[1].cpu()
    ok, ratio, used = S.holds_xu({"T": T_, "Tt": Tt[:, :M]}, model, dt, quiet=True, name=name)
    lo, hi = model["pad"]
    pad_ok = bool((_bits(Tt[:, lo:hi]) == 0).all()) and bool(torch.isnan(Tt[:, hi:]).all())
    intact = _intact(Tb, Ttb)
    print(f"  {tag}: worst/bound {ratio:.3f}  neighbours {used:.4f}/{T.SKINNY_CAPS[name]}  pad [{lo}, {hi}) zero and the rest untouched {pad_ok}  guards {intact}")
    assert ok, f"{tag}: worst/bound {ratio:.3f}, share {used}"
    assert pad_ok and intact, tag
    return ratio, used


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("case", S.XU_CASES, ids=lambda c: "M%d_K%d_Rp%d_r%d" % c)
def test_skinny_xu(case, operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    M, Kc, Rp, rank = case
    o = S.xu_operands(*case, dt)
    model = K.xu(o["X"], o["Ut"], *case, ldt=K.roundup32(M))
    Xd, Utd = _rows(o["X"], M, Kc, dt), o["Ut"].to(DEV)
    print(f"\nxu {case} {operands}: {model['plan']}")
    rc, Tb, Ttb = _xu_call(lib, Xd, Kc, Utd, M, Kc, Rp, rank, dt)
    assert rc == 0
    _hold_xu("xu_r", model, Tb, Ttb, M, dt)
    rc, Tb2, Ttb2 = _xu_call(lib, Xd, Kc, Utd, M, Kc, Rp, rank, dt, with_tt=False)      # Tt == NULL: the same T, Tt's buffer untouched
    assert rc == 0 and _same(Tb[1], Tb2[1]) and _all_nan(Ttb2) and _intact(Tb2, Ttb2)
    if rank == Rp:
        rc, Tb3, Ttb3 = _xu_call(lib, Xd, Kc, Utd, M, Kc, Rp, rank, dt, plain=True)
        assert rc == 0 and _same(Tb[1], Tb3[1]) and _same(Ttb[1][:, :M], Ttb3[1][:, :M]) and _intact(Tb3, Ttb3), "cara_skinny_xu != cara_skinny_xu_r at rank = Rp"


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("case", S.XU_LAYOUTS, ids=lambda c: "M%d_K%d_Rp%d_r%d_%s" % c)
def test_skinny_xu_layouts_of_x(case, operands):
    """ldx = K + 8 (NaN between K and ldx) and the K-panel-major X (ldx = -P, P = M and P = M + 24 with NaN rows behind M - 1) through both
    kernels: inside the bounds and the row-major call's bits"""
    lib, dt = L().lib(operands), L().act_dtype(operands)
    M, Kc, Rp, rank, layout = case
    o = S.xu_operands(M, Kc, Rp, rank, dt)
    model = K.xu(o["X"], o["Ut"], M, Kc, Rp, rank, ldt=K.roundup32(M))
    Utd = o["Ut"].to(DEV)
    rc, Tb, Ttb = _xu_call(lib, _rows(o["X"], M, Kc, dt), Kc, Utd, M, Kc, Rp, rank, dt)
    assert rc == 0
    if layout == "ldx+8":
        Xd, ldx = _rows(o["X"], M, Kc, dt, ld=Kc + 8), Kc + 8
    else:
        P = M + 24 if layout == "panels+" else M
        Xd, ldx = _panels(o["X"], M, Kc, dt, P), -P
    rc, Tb2, Ttb2 = _xu_call(lib, Xd, ldx, Utd, M, Kc, Rp, rank, dt)
    assert rc == 0
    print(f"\nxu {case} {operands}: {model['plan']['kernel']}")
    _hold_xu(layout, model, Tb2, Ttb2, M, dt)
    assert _same(Tb[1], Tb2[1]) and _same(Ttb[1][:, :M], Ttb2[1][:, :M])


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("M,ldt", S.XU_LDT)
def test_skinny_xu_pad_of_tt(M, ldt, operands):
    """ldt > roundup32(M): columns [M, roundup32(M)) zero, [roundup32(M), ldt) untouched; ldt = M = 40: the pad does not fit, the memset is
    skipped, nothing at or beyond ldt is written.  v1 (K = 224) and, where M >= 64, the sliced kernel (K = 768); NT = 1, 2 and Rp = 64"""
    lib, dt = L().lib(operands), L().act_dtype(operands)
    for Kc, Rp, rank in ((224, 32, 32), (768, 32, 16), (768, 64, 64)):
        o = S.xu_operands(M, Kc, Rp, rank, dt)
        model = K.xu(o["X"], o["Ut"], M, Kc, Rp, rank, ldt=ldt)
        assert model["pad"] == ((M, K.roundup32(M)) if ldt >= K.roundup32(M) else (M, M))
        rc, Tb, Ttb = _xu_call(lib, _rows(o["X"], M, Kc, dt), Kc, o["Ut"].to(DEV), M, Kc, Rp, rank, dt, ldt=ldt)
        assert rc == 0
        print(f"\nxu pad M={M} ldt={ldt} K={Kc} Rp={Rp} rank={rank} {operands}: {model['plan']['kernel']}")
        _hold_xu("pad", model, Tb, Ttb, M, dt)


@pytest.mark.parametrize("operands", OPERANDS)
def test_skinny_xu_refusals_write_nothing(operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    M, Kc, Rp, rank = 65, 768, 32, 16
    o = S.xu_operands(M, Kc, Rp, rank, dt)
    Xd, Utd = _rows(o["X"], M, Kc, dt, ld=Kc + 8), o["Ut"].to(DEV)
    Xp = _panels(o["X"], M, Kc, dt)
    Tb, Ttb = _buf((M, 64), dt), _buf((64, 96), dt)

    def call(**kw):
        a = dict(X=Xd, ldx=Kc + 8, Ut=Utd, T=Tb[1], Tt=Ttb[1], ldt=96, M=M, K=Kc, Rp=Rp, rank=rank)
        a.update(kw)
        return lib.cara_skinny_xu_r(_p(a["X"]), a["ldx"], _p(a["Ut"]), _p(a["T"]), _p(a["Tt"]), a["ldt"], a["M"], a["K"], a["Rp"], a["rank"], _st())
    bad = {"K % 32": dict(K=Kc - 16), "ldx < K": dict(ldx=Kc - 8), "ldx % 8": dict(ldx=Kc + 4), "-ldx < M": dict(X=Xp, ldx=-(M - 1)), "ldt < M": dict(ldt=64),
           "ldt % 8": dict(ldt=100), "rank 0": dict(rank=0), "rank > Rp": dict(rank=33), "Rp 48": dict(Rp=48, rank=48), "Rp 48 sliced": dict(Rp=48, rank=16),
           "X NULL": dict(X=None), "Ut NULL": dict(Ut=None), "T NULL": dict(T=None), "M 0": dict(M=0), "K 0": dict(K=0)}
    for what, kw in bad.items():
        assert call(**kw) != 0, what
    assert lib.cara_skinny_xu(_p(Xd), Kc + 8, _p(Utd), _p(Tb[1]), _p(Ttb[1]), 96, M, Kc, 48, _st()) != 0
    torch.cuda.synchronize()
    assert _all_nan(Tb, Ttb) and _intact(Tb, Ttb)
    assert call() == 0      # ... and the same arguments are taken once nothing is wrong with them
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Tb[1].view(-1)[:M * Rp]).all())


# --- the transposed products ----------------------------------------------------------------------------------------------------
def _slabs(lib, M, K1, Rp):
    nb = int(lib.cara_tskinny_scratch_bytes(M, K1, Rp))
    assert nb == K.ts_scratch_bytes(M, K1, Rp), (M, K1, Rp, nb)
    return _buf((nb // 4,), torch.float32)


def _red(slabs, D, cs, M, K1, Rp, Rc=0, batch=1, stride=0, wave_slabs=0):
    return L().TsReduce(slabs.data_ptr() if torch.is_tensor(slabs) else slabs, stride, D.data_ptr() if torch.is_tensor(D) else D,
                        cs.data_ptr() if cs is not None else None, batch, M, K1, Rp, Rc, wave_slabs)


def _reduce_many(lib, *entries):
    tab = (L().TsReduce * len(entries))(*entries)
    return lib.cara_tskinny_reduce_many(tab, len(entries), _st())


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("M,K1", S.TS_MK)
def test_tskinny(M, K1, operands):
    """per (Rp, rank): cara_tskinny_xtg with and without column sums, cara_tskinny_partial2_r with Xa == NULL reduced by reduce_many (Rc = 16
    where the one-r-tile form ran), the panel-major X, ldg > roundup32(M) with NaN behind roundup32(M), NaN rows of X behind row M - 1"""
    lib, dt = L().lib(operands), L().act_dtype(operands)
    m32 = K.roundup32(M)
    print(f"\ntskinny M={M} K1={K1} {operands}: chunks {K.ts_chunks(M, K1)}, steps per wave {sorted(K.ts_wave_steps(M, K1))}, kappa {K.kappa_xtg(M, K1)}")
    worst = {}
    for Rp, rank in S.ts_ranks(M, K1):
        half = Rp == 32 and rank <= 16
        o = S.ts_operands(M, K1, Rp, rank, dt)
        full_m, half_m = K.xtg(o["X"], o["Gt"], M, K1, Rp, rank), K.xtg(o["X"], o["Gt"], M, K1, Rp, rank, half=half)
        other = S.restate_xtg(o, M, K1, Rp, rank)
        ldg = m32 + (8 if rank != Rp else 0)
        Gtd = torch.full((Rp, ldg), NAN, dtype=dt, device=DEV)
        Gtd[:, :m32] = o["Gt"].to(DEV)
        Xd = _rows(o["X"], M, K1, dt, ld=K1 + (8 if Rp == 64 else 0))
        ldx = Xd.shape[1]
        sl, Db, cb = _slabs(lib, M, K1, Rp), _buf((K1, Rp), torch.float32), _buf((K1,), torch.float32)
        assert lib.cara_tskinny_xtg(_p(Xd), ldx, _p(Gtd), ldg, _p(Db[1]), _p(cb[1]), _p(sl[1]), M, K1, Rp, _st()) == 0
        torch.cuda.synchronize()
        got = {"D": Db[1].cpu(), "colsum": cb[1].cpu()}
        for name, (ok, ratio, agg) in S.holds_xtg(got, full_m, other).items():
            print(f"  xtg Rp{Rp} rank{rank} {name}: worst/bound {ratio:.3f}  rms vs other order {agg:.2f}")
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert ok, f"xtg Rp{Rp} rank{rank} {name}: worst/bound {ratio:.3f}, aggregate {agg:.2f}"
        assert _intact(sl, Db, cb)
        # column sums off: the same D, colsum's buffer untouched;  reduce_many at Rc = 0 is cara_tskinny_reduce bit for bit
        sl2, Db2, cb2 = _slabs(lib, M, K1, Rp), _buf((K1, Rp), torch.float32), _buf((K1,), torch.float32)
        assert lib.cara_tskinny_xtg(_p(Xd), ldx, _p(Gtd), ldg, _p(Db2[1]), None, _p(sl2[1]), M, K1, Rp, _st()) == 0
        Db3, cb3 = _buf((K1, Rp), torch.float32), _buf((K1,), torch.float32)
        assert _reduce_many(lib, _red(sl[1], Db3[1], cb3[1], M, K1, Rp)) == 0
        torch.cuda.synchronize()
        assert _same(Db[1], Db2[1]) and _all_nan(cb2) and _intact(sl2, Db2, cb2)
        assert _same(Db[1], Db3[1]) and _same(cb[1], cb3[1]) and _intact(Db3, cb3)
        # partial2_r with Xa == NULL from the panel-major X with finite rows behind M - 1; Rc = 16 where the one-r-tile form ran
        Xp = _panels(o["X"], M, K1, dt, P=M + 8, behind=1.0)
        sl4, Db4, cb4 = _slabs(lib, M, K1, Rp), _buf((K1, Rp), torch.float32), _buf((K1,), torch.float32)
        assert lib.cara_tskinny_partial2_r(None, 0, None, None, 0, _p(Xp), -(M + 8), _p(Gtd), _p(sl4[1]), K1, 1, ldg, M, Rp, rank, _st()) == 0
        assert _reduce_many(lib, _red(sl4[1], Db4[1], cb4[1], M, K1, Rp, Rc=16 if half else 0)) == 0
        torch.cuda.synchronize()
        got4 = {"D": Db4[1].cpu(), "colsum": cb4[1].cpu()}
        for name, (ok, ratio, agg) in S.holds_xtg(got4, half_m, other).items():
            assert ok, f"partial2_r Rp{Rp} rank{rank} {name}: worst/bound {ratio:.3f}, aggregate {agg:.2f}"
        keep = 16 if half else Rp
        assert _same(Db[1][:, :keep], Db4[1][:, :keep]) and _same(cb[1], cb4[1]), "panel-major X / rows behind M - 1 / the one-r-tile form changed the sums"
        assert _intact(sl4, Db4, cb4)
    print(f"SUMMARY tskinny M={M} K1={K1} {operands}: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("M,K1a,K1b,Rp,rank", [(33, 64, 768, 32, 32), (257, 128, 64, 32, 5), (385, 768, 128, 64, 40), (1000, 64, 128, 32, 16)])
def test_tskinny_two_problems_in_one_launch(M, K1a, K1b, Rp, rank, operands):
    """cara_tskinny_partial2 / partial2_r on two problems of different K1 (different nchunks), reduced by ONE reduce_many launch"""
    lib, dt = L().lib(operands), L().act_dtype(operands)
    half = Rp == 32 and rank <= 16
    oa, ob = S.ts_operands(M, K1a, Rp, rank, dt), S.ts_operands(M, K1b, Rp, rank, dt, seed=1)
    m32 = K.roundup32(M)
    Xa, Xb, Ga, Gb = _rows(oa["X"], M, K1a, dt), _rows(ob["X"], M, K1b, dt), oa["Gt"].to(DEV), ob["Gt"].to(DEV)
    for entry in ("partial2", "partial2_r"):
        h = half and entry == "partial2_r"
        sa, sb = _slabs(lib, M, K1a, Rp), _slabs(lib, M, K1b, Rp)
        Da, Dbb, cs = _buf((K1a, Rp), torch.float32), _buf((K1b, Rp), torch.float32), _buf((K1b,), torch.float32)
        if entry == "partial2":
            rc = lib.cara_tskinny_partial2(_p(Xa), K1a, _p(Ga), _p(sa[1]), K1a, _p(Xb), K1b, _p(Gb), _p(sb[1]), K1b, 1, m32, M, Rp, _st())
        else:
            rc = lib.cara_tskinny_partial2_r(_p(Xa), K1a, _p(Ga), _p(sa[1]), K1a, _p(Xb), K1b, _p(Gb), _p(sb[1]), K1b, 1, m32, M, Rp, rank, _st())
        assert rc == 0
        assert _reduce_many(lib, _red(sa[1], Da[1], None, M, K1a, Rp, Rc=16 if h else 0), _red(sb[1], Dbb[1], cs[1], M, K1b, Rp, Rc=16 if h else 0)) == 0
        torch.cuda.synchronize()
        print(f"\n{entry} M={M} K1=({K1a}, {K1b}) Rp{Rp} rank{rank} {operands}: chunks ({K.ts_chunks(M, K1a)}, {K.ts_chunks(M, K1b)})")
        for tag, o, K1, got in (("a", oa, K1a, {"D": Da[1].cpu()}), ("b", ob, K1b, {"D": Dbb[1].cpu(), "colsum": cs[1].cpu()})):
            model = K.xtg(o["X"], o["Gt"], M, K1, Rp, rank, colsum=tag == "b", half=h)
            for name, (ok, ratio, agg) in S.holds_xtg(got, model, S.restate_xtg(o, M, K1, Rp, rank, half=h)).items():
                print(f"  {tag} {name}: worst/bound {ratio:.3f}  rms vs other order {agg:.2f}")
                assert ok, f"{entry} {tag} {name}: worst/bound {ratio:.3f}, aggregate {agg:.2f}"
        assert _intact(sa, sb, Da, Dbb, cs)


@pytest.mark.parametrize("operands", OPERANDS)
def test_reduce_many_mixed_batches_is_reduce_bit_for_bit(operands):
    """entries of batch 1, 3 and 2 under one grid (grid.y = 3: the blocks beyond an entry's batch return), slab strides > the slabs"""
    lib, dt = L().lib(operands), L().act_dtype(operands)
    probs, keep = [], []
    for M, K1, Rp, batch, want_cs in ((129, 64, 32, 1, True), (513, 128, 64, 3, True), (33, 768, 32, 2, False)):
        nb = K.ts_scratch_bytes(M, K1, Rp)
        stride = (nb + 255) // 256 * 256 + 256
        sl = _buf((batch * stride // 4,), torch.float32)
        m32 = K.roundup32(M)
        for b in range(batch):
            o = S.ts_operands(M, K1, Rp, Rp, dt, seed=b)
            assert lib.cara_tskinny_partial(_p(_rows(o["X"], M, K1, dt)), K1, _p(o["Gt"].to(DEV)), m32, C.c_void_p(sl[1].data_ptr() + b * stride), 1 if want_cs else 0,
                                            M, K1, Rp, _st()) == 0
        D1, D2, c1, c2 = _buf((batch, K1, Rp), torch.float32), _buf((batch, K1, Rp), torch.float32), _buf((batch, K1), torch.float32), _buf((batch, K1), torch.float32)
        assert lib.cara_tskinny_reduce(_p(sl[1]), SZ(stride), _p(D1[1]), _p(c1[1]) if want_cs else None, batch, M, K1, Rp, _st()) == 0
        probs.append(_red(sl[1], D2[1], c2[1] if want_cs else None, M, K1, Rp, batch=batch, stride=stride))
        keep.append((D1, D2, c1, c2, want_cs, sl))
    assert _reduce_many(lib, *probs) == 0
    torch.cuda.synchronize()
    for D1, D2, c1, c2, want_cs, sl in keep:
        assert not torch.isnan(D1[1]).any() and _same(D1[1], D2[1]) and _intact(D1, D2, c1, c2, sl)
        assert (_same(c1[1], c2[1]) and not torch.isnan(c1[1]).any()) if want_cs else _all_nan(c1, c2)


@pytest.mark.parametrize("operands", OPERANDS)
def test_tskinny_refusals_write_nothing(operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    M, K1, Rp, rank = 33, 128, 32, 16
    o = S.ts_operands(M, K1, Rp, rank, dt)
    Xd, Gd = _rows(o["X"], M, K1, dt, ld=K1 + 8), torch.zeros(64, 72, dtype=dt, device=DEV)
    Xp = _panels(o["X"], M, K1, dt)
    sl, Db, cb = _slabs(lib, M, K1, 64), _buf((K1, 64), torch.float32), _buf((K1,), torch.float32)

    def partial(**kw):
        a = dict(X=Xd, ldx=K1 + 8, Gt=Gd, ldg=72, slabs=sl[1], K1=K1, Rp=Rp, rank=rank, M=M)
        a.update(kw)
        x, g, s = _p(a["X"]), _p(a["Gt"]), _p(a["slabs"])
        if "rank" in kw:     # (the one entry that takes the rank)
            return [lib.cara_tskinny_partial2_r(None, 0, None, None, 0, x, a["ldx"], g, s, a["K1"], 1, a["ldg"], a["M"], a["Rp"], a["rank"], _st())]
        return [lib.cara_tskinny_partial(x, a["ldx"], g, a["ldg"], s, 1, a["M"], a["K1"], a["Rp"], _st()),
                lib.cara_tskinny_partial2(x, a["ldx"], g, s, a["K1"], x, a["ldx"], g, s, a["K1"], 1, a["ldg"], a["M"], a["Rp"], _st()),
                lib.cara_tskinny_partial2_r(None, 0, None, None, 0, x, a["ldx"], g, s, a["K1"], 1, a["ldg"], a["M"], a["Rp"], a["rank"], _st()),
                lib.cara_tskinny_xtg(x, a["ldx"], g, a["ldg"], _p(Db[1]), _p(cb[1]), s, a["M"], a["K1"], a["Rp"], _st())]
    bad = {"K1 % 64": dict(K1=96), "ldg < roundup32(M)": dict(ldg=56), "ldg % 8": dict(ldg=68), "Rp 48": dict(Rp=48), "ldx < K1": dict(ldx=K1 - 8), "ldx % 8": dict(ldx=K1 + 4),
           "-ldx < M": dict(X=Xp, ldx=-(M - 1)), "X NULL": dict(X=None), "Gt NULL": dict(Gt=None), "slabs NULL": dict(slabs=None), "M 0": dict(M=0)}
    for what, kw in bad.items():
        assert all(rc != 0 for rc in partial(**kw)), what
    for what, kw in {"rank 0": dict(rank=0), "rank > Rp": dict(rank=33)}.items():
        assert partial(**kw)[0] != 0, what
    assert lib.cara_tskinny_xtg(_p(Xd), K1 + 8, _p(Gd), 72, None, None, _p(sl[1]), M, K1, Rp, _st()) != 0
    for m, k, r in ((0, K1, Rp), (M, 96, Rp), (M, K1, 48)):
        assert int(lib.cara_tskinny_scratch_bytes(m, k, r)) == 0
    s, D = sl[1].data_ptr(), Db[1].data_ptr()
    red = {"slabs misaligned": _red(s + 4, D, None, M, K1, Rp), "D misaligned": _red(s, D + 4, None, M, K1, Rp), "slab_stride misaligned": _red(s, D, None, M, K1, Rp, stride=4),
           "Rc 8": _red(s, D, None, M, K1, Rp, Rc=8), "Rc 16 at Rp 64": _red(s, D, None, M, K1, 64, Rc=16), "wave_slabs with Rc 0": _red(s, D, None, M, K1, Rp, wave_slabs=1),
           "wave_slabs with Rc 32": _red(s, D, None, M, K1, Rp, Rc=32, wave_slabs=2), "wave_slabs < 0": _red(s, D, None, M, K1, Rp, Rc=16, wave_slabs=-1),
           "batch 0": _red(s, D, None, M, K1, Rp, batch=0), "K1 % 64": _red(s, D, None, M, 96, Rp), "Rp 48": _red(s, D, None, M, K1, 48),
           "slabs NULL": _red(None, D, None, M, K1, Rp), "D NULL": _red(s, None, None, M, K1, Rp)}
    for what, e in red.items():
        assert _reduce_many(lib, e) != 0, what
        assert _reduce_many(lib, _red(s, D, None, M, K1, Rp), e) != 0, what + " (second entry)"
    good = _red(s, D, None, M, K1, Rp)
    tab = (L().TsReduce * (K.TS_REDUCE_MAX + 1))(*([good] * (K.TS_REDUCE_MAX + 1)))
    assert lib.cara_tskinny_reduce_many(tab, K.TS_REDUCE_MAX + 1, _st()) != 0 and lib.cara_tskinny_reduce_many(tab, 0, _st()) != 0
    assert lib.cara_tskinny_reduce_many(None, 1, _st()) != 0
    assert lib.cara_tskinny_reduce(_p(sl[1]), SZ(0), None, None, 1, M, K1, Rp, _st()) != 0 and lib.cara_tskinny_reduce(_p(sl[1]), SZ(0), _p(Db[1]), None, 1, M, K1, 48, _st()) != 0
    torch.cuda.synchronize()
    assert _all_nan(sl, Db, cb) and _intact(sl, Db, cb)
    assert all(rc == 0 for rc in partial()) and _reduce_many(lib, good) == 0      # ... and the same arguments are taken once nothing is wrong with them
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Db[1].view(-1)[:K1 * Rp]).all())


# --- cara_gemm_tn_f32 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("M,N", S.TN_MN)
def test_gemm_tn(M, N, operands):
    """lda = M + 8, ldb = N + 16 (NaN in the padding and in the rows behind K - 1), ldc = N + 4: every slab inside the bound over ITS rows,
    the columns between N and ldc and the gap between the slabs untouched"""
    lib, dt = L().lib(operands), L().act_dtype(operands)
    lda, ldb, ldc = M + 8, N + 16, N + 4
    for Kc in S.TN_K:
        o = S.tn_operands(M, N, Kc, dt)
        Ad, Bd = _rows(o["At"], Kc, M, dt, ld=lda, extra=40), _rows(o["Bt"], Kc, N, dt, ld=ldb, extra=40)
        for ns in S.TN_NSLAB:
            stride = M * ldc + 8
            Cb = _buf((ns, stride), torch.float32)
            rc = lib.cara_gemm_tn_f32(_p(Ad), lda, _p(Bd), ldb, _p(Cb[1]), ldc, M, N, Kc, ns, SZ(stride), _st())
            torch.cuda.synchronize()
            if K.tn_kslab(Kc, ns) is None:
                assert rc != 0 and _all_nan(Cb) and _intact(Cb), (Kc, ns)
                continue
            assert rc == 0, (Kc, ns)
            out = Cb[1].cpu()
            tiles = out[:, :M * ldc].view(ns, M, ldc)
            model, other = K.tn(o["At"], o["Bt"], M, N, Kc, ns), S.restate_tn(o, M, N, Kc, ns)
            print(f"\ntn M={M} N={N} K={Kc} nslab={ns} kslab={K.tn_kslab(Kc, ns)} {operands}")
            for name, (ok, ratio, agg) in S.holds_tn([tiles[z, :, :N] for z in range(ns)], model, other, quiet=False).items():
                assert ok, f"K={Kc} nslab={ns} {name}: worst/bound {ratio:.3f}, aggregate {agg:.2f}"
            assert bool(torch.isnan(tiles[:, :, N:]).all()) and bool(torch.isnan(out[:, M * ldc:]).all()) and _intact(Cb)


@pytest.mark.parametrize("operands", OPERANDS)
def test_gemm_tn_refusals_write_nothing(operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    M, N, Kc = 128, 128, 95
    o = S.tn_operands(M, N, Kc, dt)
    Ad, Bd = _rows(o["At"], Kc, M, dt, ld=M + 8, extra=40), _rows(o["Bt"], Kc, N, dt, ld=N + 16, extra=40)
    Cb = _buf((3, M * (N + 4)), torch.float32)

    def call(**kw):
        a = dict(At=Ad, lda=M + 8, Bt=Bd, ldb=N + 16, C=Cb[1], ldc=N + 4, M=M, N=N, K=Kc, nslab=2, stride=M * (N + 4))
        a.update(kw)
        return lib.cara_gemm_tn_f32(_p(a["At"]), a["lda"], _p(a["Bt"]), a["ldb"], _p(a["C"]), a["ldc"], a["M"], a["N"], a["K"], a["nslab"], SZ(a["stride"]), _st())
    bad = {"M % 128": dict(M=120), "N % 128": dict(N=64), "lda < M": dict(lda=120), "lda % 8": dict(lda=M + 4), "ldb < N": dict(ldb=120), "ldb % 8": dict(ldb=N + 4),
           "ldc < N": dict(ldc=124), "ldc % 4": dict(ldc=N + 2), "empty last slab": dict(K=64, nslab=3), "empty last slab, K = 32": dict(K=32, nslab=2),
           "slab_stride < M ldc": dict(stride=M * (N + 4) - 4), "nslab 0": dict(nslab=0), "nslab 65536": dict(nslab=65536), "K 0": dict(K=0),
           "2^32 bytes of At": dict(K=(1 << 32) // ((M + 8) * 2) + 1, nslab=1), "At NULL": dict(At=None), "Bt NULL": dict(Bt=None), "C NULL": dict(C=None)}
    for what, kw in bad.items():
        assert call(**kw) != 0, what
    torch.cuda.synchronize()
    assert _all_nan(Cb) and _intact(Cb)
    assert call() == 0 and call(nslab=1, stride=0) == 0
    torch.cuda.synchronize()
    assert _intact(Cb)


# --- cara_linear_fwd / cara_linear_bwd --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("M", S.LIN_M)
@pytest.mark.parametrize("geom", S.LIN_GEOMS, ids=lambda g: "in%d_out%d_r%d_Rp%d" % g)
def test_linear_fwd_bwd(geom, M, operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    in_, out_, rank, Rp = geom
    o = S.lin_operands(geom, M, dt)
    d = {k: o[k].to(DEV) for k in ("W", "Wt", "Ut", "U", "Vs", "Vst", "bias", "aux", "rowscale")}
    lin = L().Linear()
    lin.W, lin.Wt, lin.Ut, lin.U, lin.Vs, lin.Vst, lin.bias = (_p(d[k]) for k in ("W", "Wt", "Ut", "U", "Vs", "Vst", "bias"))
    setattr(lin, "in", in_)
    lin.out, lin.Rp, lin.rank = out_, Rp, rank
    ldt = K.roundup32(M)
    Xd, dYd = _rows(o["X"], M, in_, dt), _rows(o["dY"], M, out_, dt)
    print(f"\nlinear {geom} M={M} {operands}")
    Tt_dev = None
    for epi, ydt in ((L().EPI_BF16, dt), (L().EPI_RESID, torch.float32)):
        Tb, Ttb, Yb = _buf((M, Rp), dt), _buf((Rp, ldt), dt), _buf((M, out_), ydt)
        resid = epi == L().EPI_RESID
        rc = lib.cara_linear_fwd(C.byref(lin), _p(Xd), in_, M, _p(Tb[1]), _p(Ttb[1]), ldt, epi, _p(Yb[1]), 0, None, _p(d["aux"]) if resid else None,
                                 _p(d["rowscale"]) if resid else None, o["rps"] if resid else 0, _st())
        torch.cuda.synchronize()
        assert rc == 0
        T_dev = Tb[1].cpu()
        m = K.linear_fwd(o["X"], o["W"], o["bias"], o["Ut"], o["Vs"], M, Rp, rank, G.EPI_RESID if resid else G.EPI_BF16, dt, T_dev, ldt,
                         aux=o["aux"] if resid else None, rowscale=o["rowscale"] if resid else None, rows_per_sample=o["rps"])
        _hold_xu("T", m, Tb, Ttb, M, dt)
        if resid:
            ok, ratio, agg = S.check_32("Y resid", Yb[1].cpu(), m["Y"], S.restate_lin_y(o, M, T_dev), o["fam"])
        else:
            ok, ratio, agg = S.check_16("Y", Yb[1].cpu(), m["Y"], dt, T.GEMM_CAPS["bf16"])
        assert ok and _intact(Yb), f"Y epi {epi}: worst/bound {ratio:.3f}, {agg}"
        Tt_dev = Ttb[1].clone()
    Gb, Gtb, dXb = _buf((M, Rp), dt), _buf((Rp, ldt), dt), _buf((M, in_), dt)
    su, sv = _slabs(lib, M, in_, Rp), _slabs(lib, M, out_, Rp)
    dU, dVs, dc = _buf((in_, Rp), torch.float32), _buf((out_, Rp), torch.float32), _buf((out_,), torch.float32)
    rc = lib.cara_linear_bwd(C.byref(lin), _p(dYd), out_, _p(Xd), in_, _p(Tt_dev), M, _p(Gb[1]), _p(Gtb[1]), ldt, _p(dXb[1]), 0, _p(su[1]), _p(sv[1]),
                             _p(dU[1]), _p(dVs[1]), _p(dc[1]), _st())
    torch.cuda.synchronize()
    assert rc == 0
    G_dev, Gt_dev, Tt_h = Gb[1].cpu(), Gtb[1].cpu(), Tt_dev.cpu()
    m = K.linear_bwd(o["dY"], o["X"], o["Wt"], o["U"], o["Vst"], M, Rp, rank, dt, G_dev, Gt_dev, Tt_h, ldt)
    _hold_xu("G'", {"T": m["G"], "pad": m["pad"]}, Gb, Gtb, M, dt)
    ok, ratio, used = S.check_16("dX", dXb[1].cpu(), m["dX"], dt, T.GEMM_CAPS["bf16"])
    assert ok, f"dX: worst/bound {ratio:.3f}, share {used}"
    half = Rp == 32 and rank <= 16
    ru = S.restate_xtg({"X": o["X"], "Gt": Gt_dev}, M, in_, Rp, rank, half=half)
    rv = S.restate_xtg({"X": o["dY"], "Gt": Tt_h}, M, out_, Rp, rank, half=half)
    res = {"dU": S.holds_xtg({"D": dU[1].cpu()}, {"D": m["dU"]}, ru, quiet=False)["D"],
           **{n: r for n, r in zip(("dVs", "dc"), S.holds_xtg({"D": dVs[1].cpu(), "colsum": dc[1].cpu()}, {"D": m["dVs"], "colsum": m["dc"]}, rv, quiet=False).values())}}
    for name, (ok, ratio, agg) in res.items():
        assert ok, f"{name}: worst/bound {ratio:.3f}, aggregate {agg:.2f}"
    assert _intact(dXb, su, sv, dU, dVs, dc)
    # the refusals of tests/test_kernels_gpu.py::test_one_adapted_linear_per_call, and a bwd that asks for dX without W^T: nothing written
    bad, Yb = L().Linear(), _buf((M, out_), dt)
    assert lib.cara_linear_fwd(C.byref(bad), _p(Xd), in_, M, _p(Gb[1]), None, ldt, L().EPI_BF16, _p(Yb[1]), 0, None, None, None, 0, _st()) != 0
    lin.Wt = None
    dU2 = _buf((in_, Rp), torch.float32)
    assert lib.cara_linear_bwd(C.byref(lin), _p(dYd), out_, _p(Xd), in_, _p(Tt_dev), M, _p(Gb[1]), _p(Gtb[1]), ldt, _p(dXb[1]), 0, _p(su[1]), _p(sv[1]),
                               _p(dU2[1]), _p(dVs[1]), _p(dc[1]), _st()) != 0
    torch.cuda.synchronize()
    assert _all_nan(Yb, dU2) and _intact(Yb, dU2) and _same(Gb[1].cpu(), G_dev)
