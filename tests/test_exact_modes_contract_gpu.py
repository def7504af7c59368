"""The kernels of dropout_exact.hip (weight_dropout = "exact") and dense_delta.hip (cp_length 2) on the device, in both operand
builds, held to the derived bounds of oracle/exact_modes_model.py (proven attainable on the host by tests/test_exact_modes_model.py,
whose inputs and float64 models are shared here).  Python refuses the two modes in fp16, so in that build this is coverage of the
C ABI only: both libraries export the entry points, with the operand type of the build.

cara_materialize_merge: the interval rule and the cap of tests/tolerances.py (EXACT_CAPS), with W and with W == NULL (dropped
elements +0 in bits).  cara_dropout_grad_contract, cara_colsum_bf16, cara_dense_delta_grad: every element under hold_f32 and the
aggregate rule against the host's other-order restatement; two calls the same bits; a dW / X that the 16-byte loads cannot serve
takes the scalar path and gives the aligned call's bits.  cara_dense_delta_materialize: Dm under the interval rule and the cap, Dmt
bitwise its transpose.  cara_sum_slabs_f32: bitwise.  Everywhere outputs and scratch are pre-filled with NaN, GUARD sentinel words
sit behind each of them, padding and gaps of the inputs hold NaN, and figures are printed (-s) before they are asserted.  Refusals
return CARA_E_ARG (0 bytes from the scratch-size entry points) and write nothing.  docs/findings/exact_modes_contract.md holds the
tables."""
import ctypes as C

import pytest
import torch

from oracle import exact_modes_model as E
from tests import exact_modes_common as S
from tests.test_exact_modes_model import (colsum_model, contract_inputs, contract_model, contract_rows, dd_inputs, dd_models, dd_rows,
                                          linear_inputs, merge_model)
from tests.test_kernels_gpu import DEV, L
from tests.test_small_kernels_gpu import GUARD, is_sentinel, sentinel

pytestmark = pytest.mark.gpu

OPERANDS = ["bf16", "fp16"]
E_ARG = 1
NAN = float("nan")


def _guarded(n, dtype):
    """n NaNs followed by GUARD sentinel words -> (whole allocation, the first n)"""
    full = sentinel((n + GUARD,), dtype)
    full[:n] = NAN
    return full, full[:n]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _intact(*pairs):
    return all(is_sentinel(full[len(live):]) for full, live in pairs)


def _p(t):
    return L().ptr(t)


def _merge(lib, W, Um, Vs, Rp, out, inn, p, seed, lin, Weff):
    return lib.cara_materialize_merge(_p(W), _p(Um), _p(Vs), Rp, out, inn, C.c_float(p), C.c_uint(seed), C.c_uint(lin), _p(Weff), L().stream())


def _contract(lib, dW, nslab, stride, Um, Vs, Rp, out, inn, p, seed, lin, dU, dVs, scratch):
    return lib.cara_dropout_grad_contract(_p(dW), nslab, C.c_size_t(stride), _p(Um), _p(Vs), Rp, out, inn, C.c_float(p), C.c_uint(seed), C.c_uint(lin),
                                          _p(dU), _p(dVs), _p(scratch), L().stream())


class Contract:
    """one (shape, Rp)'s guarded, NaN-filled outputs and scratch"""

    def __init__(self, lib, out, inn, Rp):
        self.lib, self.out, self.inn, self.Rp = lib, out, inn, Rp
        self.nscratch = int(lib.cara_dropout_grad_scratch_bytes(out, inn, Rp)) // 4
        assert self.nscratch == ((inn + 63) // 64 * out + (out + 63) // 64 * inn) * Rp
        self.fresh()

    def fresh(self):
        self.dU, self.dVs, self.scratch = _guarded(self.inn * self.Rp, torch.float32), _guarded(self.out * self.Rp, torch.float32), _guarded(self.nscratch, torch.float32)

    def call(self, slabs, stride, Um, Vs, p, seed, lin, offset=0):
        """slabs [nslab, out, in] on the host -> laid out `stride` floats apart from float `offset` of a NaN-filled buffer"""
        nslab, n = slabs.shape[0], self.out * self.inn
        buf = torch.full((offset + nslab * stride + 4,), NAN, device=DEV)
        for z in range(nslab):
            buf[offset + z * stride:offset + z * stride + n] = slabs[z].reshape(-1).to(DEV)
        L().check(_contract(self.lib, buf[offset:], nslab, stride, Um, Vs, self.Rp, self.out, self.inn, p, seed, lin, self.dU[1], self.dVs[1], self.scratch[1]), "contract")
        torch.cuda.synchronize()
        return {"dU": self.dU[1].view(self.inn, self.Rp).cpu(), "dVs": self.dVs[1].view(self.out, self.Rp).cpu()}

    def intact(self):
        return _intact(self.dU, self.dVs, self.scratch)


# --- cara_materialize_merge, cara_dropout_grad_contract ------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("Rp", S.RPS)
@pytest.mark.parametrize("shape", S.SHAPES, ids=S.sid)
def test_merge_and_contract(shape, Rp, operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    out, inn = shape
    run_c = Contract(lib, out, inn, Rp)
    worst = {}
    for run in S.runs():
        p, seed, lin, family, nslab, gap = run
        W, Um, Vs = linear_inputs(shape, Rp, family, operands)
        Wd, Ud, Vd = W.to(DEV), Um.to(DEV), Vs.to(DEV)
        for with_w in (True, False):
            full, Weff = _guarded(out * inn, dt)
            L().check(_merge(lib, Wd if with_w else None, Ud, Vd, Rp, out, inn, p, seed, lin, Weff), "merge")
            torch.cuda.synchronize()
            name = "merge_Weff" if with_w else "merge_Dm"
            print(f"\n{S.sid(shape)} Rp{Rp} {operands} p={p} seed={seed} lin={lin} {family} {name}")
            ok, ratio, used = S.holds_merge(name, Weff.view(out, inn).cpu(), merge_model(shape, Rp, run, operands, with_w), dt, with_w, quiet=False)
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert ok, f"{name} {run}: worst/bound {ratio:.3f}, share {used}"
            assert _intact((full, Weff))
        slabs = contract_inputs(shape, run)
        stride = out * inn if gap == 0 else (out * inn + gap + 3) // 4 * 4
        run_c.fresh()
        got = run_c.call(slabs, stride, Ud, Vd, p, seed, lin)
        other = S.restate_contract(slabs, Um, Vs, p, seed, lin)
        print(f"{S.sid(shape)} Rp{Rp} {operands} p={p} seed={seed} lin={lin} {family} nslab={nslab} stride={stride}")
        res = S.holds_f32(contract_model(shape, Rp, run, operands), got, other, contract_rows(shape, family), quiet=False)
        intact = run_c.intact()
        for name, (ok, ratio, agg) in res.items():
            worst[name] = max(worst.get(name, 0.0), ratio)
            worst[name + "_agg"] = max(worst.get(name + "_agg", 0.0), agg)
            assert ok, f"{name} {run}: worst/bound {ratio:.3f}, aggregate {agg:.2f}"
        assert intact
        run_c.fresh()
        again = run_c.call(slabs, stride, Ud, Vd, p, seed, lin)
        assert all(torch.equal(_bits(got[k]), _bits(again[k])) for k in got), "two calls differ"
    print(f"\nSUMMARY {S.sid(shape)} Rp{Rp} {operands}: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("operands", OPERANDS)
def test_contract_serves_a_dW_its_16_byte_loads_cannot(operands):
    """(130, 260): in % 4 == 0.  slab_stride = out in + 1 (the second slab 4 bytes off a 16-byte boundary) and dW offset by one float:
    the entry point takes the scalar path, which adds in the same order -- inside the same bounds, and the aligned call's bits"""
    lib = L().lib(operands)
    shape, Rp = (130, 260), 32
    out, inn = shape
    run = next(r for r in S.runs() if r[4] == 2 and r[0] > 0)
    p, seed, lin, family, nslab, _ = run
    _, Um, Vs = linear_inputs(shape, Rp, family, operands)
    Ud, Vd = Um.to(DEV), Vs.to(DEV)
    slabs = contract_inputs(shape, run)
    c = Contract(lib, out, inn, Rp)
    aligned = c.call(slabs, out * inn, Ud, Vd, p, seed, lin)
    other = S.restate_contract(slabs, Um, Vs, p, seed, lin)
    for what, stride, offset in (("odd stride", out * inn + 1, 0), ("offset dW", out * inn, 1), ("both", out * inn + 1, 1)):
        c.fresh()
        got = c.call(slabs, stride, Ud, Vd, p, seed, lin, offset=offset)
        print(f"\n{what} {operands}")
        for name, (ok, ratio, agg) in S.holds_f32(contract_model(shape, Rp, run, operands), got, other, contract_rows(shape, family), quiet=False).items():
            assert ok, f"{what} {name}: worst/bound {ratio:.3f}, aggregate {agg:.2f}"
        assert c.intact()
        assert all(torch.equal(_bits(got[k]), _bits(aligned[k])) for k in got), what


# --- cara_colsum_bf16 -------------------------------------------------------------------------------------------------------
def _colsum(lib, X, M, N, ld, dt, offset=0):
    """X [M, N] on the host inside a NaN-filled [M + 8, ld] allocation that starts `offset` elements into its buffer"""
    buf = torch.full((offset + (M + 8) * ld,), NAN, dtype=dt, device=DEV)
    buf[offset:].view(M + 8, ld)[:M, :N] = X[:M, :N].to(DEV)
    nscratch = int(lib.cara_colsum_scratch_bytes(N)) // 4
    assert nscratch == 256 * N
    o, scratch = _guarded(N, torch.float32), _guarded(nscratch, torch.float32)
    L().check(lib.cara_colsum_bf16(_p(buf[offset:]), ld, M, N, _p(o[1]), _p(scratch[1]), L().stream()), "colsum")
    torch.cuda.synchronize()
    return o[1].cpu(), _intact(o, scratch)


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("case", S.COLSUM, ids=S.sid)
def test_colsum(case, operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    M, N, ld = case
    X, (v, d, chunks) = colsum_model(case, operands)
    assert chunks == E.colsum_chunks(M, N)
    if case == S.COLSUM_EMPTY:
        assert E.colsum_empty_chunks(M, N) >= 1
    got, intact = _colsum(lib, X, M, N, ld, dt)
    print(f"\ncolsum {S.sid(case)} {operands}: chunks {chunks}, empty {E.colsum_empty_chunks(M, N)}, guards intact {intact}")
    ok, ratio, agg = S.holds_f32({"colsum": (v, d)}, {"colsum": got}, {"colsum": S.restate_colsum(X, M, N)}, quiet=False)["colsum"]
    assert ok, f"worst/bound {ratio:.3f}, aggregate {agg:.2f}"
    assert intact
    again, _ = _colsum(lib, X, M, N, ld, dt)
    assert torch.equal(_bits(got), _bits(again))
    if ld % 8 == 0:      # X one element off a 16-byte boundary: the scalar path, the same order, the same bits
        off, intact = _colsum(lib, X, M, N, ld, dt, offset=1)
        assert intact and torch.equal(_bits(got), _bits(off)), "X offset by one element"


# --- dense delta --------------------------------------------------------------------------------------------------------------
def _dd_geom(geom, **over):
    depth, dim, rank = geom
    f = dict(depth=depth, dim=dim, heads=4, rank=rank, Rp=64 if rank > 32 else 32, scale=S.S, cp_length=2)
    f.update(over)
    return L().Geom(**f)


class Dense:
    def __init__(self, lib, geom, dt, A1, A2, R1, dD):
        self.lib, self.geom, self.dt = lib, geom, dt
        depth, dim, R = geom
        self.g = _dd_geom(geom)
        self.d = {"A1": A1.to(DEV).contiguous(), "A2": A2.to(DEV).contiguous(), "R1": R1.to(DEV).contiguous()}
        self.dD = dD.to(DEV).contiguous()
        self.cps = L().CpPtrs(**{k: _p(v) for k, v in self.d.items()})
        self.nscratch = int(lib.cara_dense_delta_grad_scratch_bytes(C.byref(self.g))) // 4
        assert self.nscratch == dim * dim // 256 * 3 * depth * R
        self.fresh()

    def fresh(self):
        depth, dim, R = self.geom
        n = depth * 3 * dim * dim
        self.Dm, self.Dmt = _guarded(n, self.dt), _guarded(n, self.dt)
        self.grads = {k: _guarded(v.numel(), torch.float32) for k, v in self.d.items()}
        self.scratch = _guarded(self.nscratch, torch.float32)
        self.gps = L().CpPtrs(**{k: _p(v[1]) for k, v in self.grads.items()})

    def materialize(self):
        depth, dim, R = self.geom
        L().check(self.lib.cara_dense_delta_materialize(C.byref(self.g), C.byref(self.cps), _p(self.Dm[1]), _p(self.Dmt[1]), L().stream()), "materialize")
        torch.cuda.synchronize()
        return self.Dm[1].view(depth, 3 * dim, dim).cpu(), self.Dmt[1].view(depth, dim, 3 * dim).cpu()

    def grad(self):
        L().check(self.lib.cara_dense_delta_grad(C.byref(self.g), C.byref(self.cps), _p(self.dD), C.byref(self.gps), _p(self.scratch[1]), L().stream()), "dense delta grad")
        torch.cuda.synchronize()
        return {k: v[1].view(self.d[k].shape).cpu() for k, v in self.grads.items()}

    def intact(self):
        return _intact(self.Dm, self.Dmt, self.scratch, *self.grads.values())

    def untouched(self):
        return all(_all_nan(v[1]) for v in (self.Dm, self.Dmt, self.scratch, *self.grads.values()))


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("geom", S.DD_GEOMS, ids=S.sid)
def test_dense_delta(geom, operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    depth, dim, R = geom
    for early in ((False, True) if depth < 64 else (False,)):
        A1, A2, R1, dD = dd_inputs(geom, early)
        mat, grad = dd_models(geom, early)
        run = Dense(lib, geom, dt, A1, A2, R1, dD)
        Dm, Dmt = run.materialize()
        print(f"\ndense delta {S.sid(geom)} {operands} early={early}")
        ok, ratio, used = S.holds_dd_materialize((Dm, Dmt), mat, dt, quiet=False)
        assert ok, f"Dm: worst/bound {ratio:.3f}, share {used}"
        got = run.grad()
        other = S.restate_dd_grad(A1, A2, R1, dD, S.S, dim)
        res = S.holds_f32(grad, got, other, dd_rows(geom), quiet=False)
        intact = run.intact()
        print(f"  guards intact {intact}")
        for name, (ok, ratio, agg) in res.items():
            assert ok, f"d{name}: worst/bound {ratio:.3f}, aggregate {agg:.2f}"
        assert intact
        run.fresh()
        Dm2, Dmt2 = run.materialize()
        again = run.grad()
        assert torch.equal(_bits(Dm), _bits(Dm2)) and torch.equal(_bits(Dmt), _bits(Dmt2))
        assert all(torch.equal(_bits(got[k]), _bits(again[k])) for k in got), "two calls differ"


# --- cara_sum_slabs_f32 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
def test_sum_slabs_bitwise(operands):
    lib = L().lib(operands)
    count, stride = S.SLAB_COUNT, S.SLAB_STRIDE
    for n in S.SLAB_NS:
        x = torch.randn(n, count, generator=torch.Generator().manual_seed(n)) * (3.0 ** torch.arange(n).float())[:, None]
        buf = torch.full((n, stride), NAN, device=DEV)
        buf[:, :count] = x.to(DEV)
        full, out = _guarded(count, torch.float32)
        L().check(lib.cara_sum_slabs_f32(_p(buf), n, C.c_size_t(stride), C.c_size_t(count), _p(out), L().stream()), "sum slabs")
        torch.cuda.synchronize()
        assert torch.equal(_bits(out.cpu()), _bits(E.sum_slabs(x, n))), n
        assert _intact((full, out))


# --- refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
def test_refusals_return_e_arg_and_write_nothing(operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    st = L().stream
    out, inn, Rp = 65, 63, 32
    run = S.runs()[4]
    p, seed, lin, family = run[:4]
    W, Um, Vs = (t.to(DEV) for t in linear_inputs((out, inn), Rp, family, operands))
    full, Weff = _guarded(out * inn, dt)
    c = Contract(lib, out, inn, Rp)
    dW = contract_inputs((out, inn), run)[0].to(DEV).contiguous()

    def merge(**o):
        a = dict(W=W, U=Um, Vs=Vs, Rp=Rp, out=out, inn=inn, p=p, Weff=Weff)
        a.update(o)
        return _merge(lib, a["W"], a["U"], a["Vs"], a["Rp"], a["out"], a["inn"], a["p"], seed, lin, a["Weff"])

    def contract(**o):
        a = dict(dW=dW, nslab=1, U=Um, Vs=Vs, Rp=Rp, out=out, inn=inn, p=p, dU=c.dU[1], dVs=c.dVs[1], scratch=c.scratch[1])
        a.update(o)
        return _contract(lib, a["dW"], a["nslab"], out * inn, a["U"], a["Vs"], a["Rp"], a["out"], a["inn"], a["p"], seed, lin, a["dU"], a["dVs"], a["scratch"])
    bad = [dict(Rp=48), dict(p=1.0), dict(p=-0.1), dict(p=NAN), dict(out=0), dict(inn=0), dict(out=65536, inn=65536), dict(U=None), dict(Vs=None)]
    for o in bad + [dict(Weff=None)]:
        assert merge(**o) == E_ARG, ("merge", o)
    for o in bad + [dict(nslab=0), dict(nslab=-1), dict(dW=None), dict(dU=None), dict(dVs=None), dict(scratch=None)]:
        assert contract(**o) == E_ARG, ("contract", o)
    for o, i, r in ((0, inn, Rp), (out, 0, Rp), (out, inn, 0)):
        assert int(lib.cara_dropout_grad_scratch_bytes(o, i, r)) == 0

    M, N, ld = 20, 24, 24
    X = torch.ones(M, ld, dtype=dt, device=DEV)
    cs, css = _guarded(N, torch.float32), _guarded(256 * N, torch.float32)
    for a in ((X, N - 1, M, N, cs[1], css[1]), (X, ld, 0, N, cs[1], css[1]), (X, ld, M, 0, cs[1], css[1]), (None, ld, M, N, cs[1], css[1]),
              (X, ld, M, N, None, css[1]), (X, ld, M, N, cs[1], None)):
        assert lib.cara_colsum_bf16(_p(a[0]), a[1], a[2], a[3], _p(a[4]), _p(a[5]), st()) == E_ARG, a[1:4]

    geom = (2, 128, 3)
    d = Dense(lib, geom, dt, *dd_inputs(geom, False))
    g = C.byref

    def dense(gm=None, cps=None, dD=True, gps=None, scratch=True, Dm=True, Dmt=True, mat=True, grad=True):
        gm = gm or d.g
        rc = []
        if mat:
            rc.append(lib.cara_dense_delta_materialize(g(gm), g(cps or d.cps), _p(d.Dm[1]) if Dm else None, _p(d.Dmt[1]) if Dmt else None, st()))
        if grad:
            rc.append(lib.cara_dense_delta_grad(g(gm), g(cps or d.cps), _p(d.dD) if dD else None, g(gps or d.gps), _p(d.scratch[1]) if scratch else None, st()))
        return all(r == E_ARG for r in rc)
    for what, over in {"cp_length 3": dict(cp_length=3), "cp_length 4": dict(cp_length=4), "dim 192": dict(dim=192), "depth 65": dict(depth=65),
                       "depth 0": dict(depth=0), "rank 0": dict(rank=0), "rank 65": dict(rank=65)}.items():
        gm = _dd_geom(geom, **over)
        assert dense(gm), what
        assert int(lib.cara_dense_delta_grad_scratch_bytes(g(gm))) == 0, what
    for name in ("A1", "A2", "R1"):
        assert dense(cps=L().CpPtrs(**{k: (None if k == name else _p(v)) for k, v in d.d.items()})), name
        assert dense(gps=L().CpPtrs(**{k: (None if k == name else _p(v[1])) for k, v in d.grads.items()}), mat=False), "gradient of " + name
    assert dense(dD=False, mat=False) and dense(scratch=False, mat=False) and dense(Dm=False, grad=False) and dense(Dmt=False, grad=False)
    slabs = torch.ones(2, 16, device=DEV)
    so = _guarded(16, torch.float32)
    sz = C.c_size_t
    assert lib.cara_sum_slabs_f32(_p(slabs), 2, sz(16), sz(0), _p(so[1]), st()) == E_ARG
    assert lib.cara_sum_slabs_f32(_p(slabs), 0, sz(16), sz(16), _p(so[1]), st()) == E_ARG
    assert lib.cara_sum_slabs_f32(None, 2, sz(16), sz(16), _p(so[1]), st()) == E_ARG
    assert lib.cara_sum_slabs_f32(_p(slabs), 2, sz(16), sz(16), None, st()) == E_ARG
    torch.cuda.synchronize()
    assert _all_nan(Weff) and _intact((full, Weff))
    assert all(_all_nan(v[1]) for v in (c.dU, c.dVs, c.scratch, cs, css, so)) and c.intact() and _intact(cs, css, so)
    assert d.untouched() and d.intact()
    # ... and the same arguments are taken once nothing is wrong with them
    assert merge() == 0 and contract() == 0
    assert lib.cara_colsum_bf16(_p(X), ld, M, N, _p(cs[1]), _p(css[1]), st()) == 0
    torch.cuda.synchronize()
    assert bool((cs[1] == M).all())
    d.materialize()
    assert set(d.grad()) == {"A1", "A2", "R1"}
