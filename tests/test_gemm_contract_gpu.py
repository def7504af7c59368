"""The GEMM family on the device, in both operand builds, held to the derived bounds of oracle/gemm_model.py (proven attainable on the
host by tests/test_gemm_model.py, whose case builders run here).  Every case first asserts the plan it was written for
(cara_debug_gemm_plan with the case's real arguments: family, tile rows, threads, nt, flags), so that a policy change fails the test
instead of moving it onto another kernel; then every 16-bit output is held to hold_16 and its cap, every fp32 output to hold_f32
and the aggregate rule, Tt_out to T_out transposed bit for bit, and every output sits in an allocation with sentinel rows and
sentinel columns N .. ldc that must be intact afterwards.  Figures are printed (-s) before they are asserted;
docs/findings/gemm_contract.md holds the tables."""
import ctypes as C

import pytest
import torch

from oracle import gemm_model as G
from tests import gemm_common as S
from tests import tolerances as T
from tests.test_kernels_gpu import DEV, L
from tests.test_small_kernels_gpu import GUARD, sentinel, is_sentinel

pytestmark = pytest.mark.gpu

OPERANDS = ["bf16", "fp16"]
_other = {}


def _guarded(rows, cols, ld, dtype, batch=1):
    """-> (whole allocation [batch, rows + GUARD, ld] of sentinels, its [rows, cols] view(s))"""
    full = sentinel((batch, rows + GUARD, ld), dtype)
    return full, (full[0, :rows, :cols] if batch == 1 else full[:, :rows, :cols])


def _intact(full, rows, cols):
    return is_sentinel(full[:, rows:]) and (cols == full.shape[2] or is_sentinel(full[:, :rows, cols:]))


class Launch:
    """the arguments of one case on the device, every output guarded"""

    def __init__(self, c, o, operands, riders=True):
        self.c, self.lib, self.dt = c, L().lib(operands), L().act_dtype(operands)
        p = L().ptr
        dt = self.dt
        d = self.d = {k: v.to(DEV).contiguous() for k, v in o.items() if torch.is_tensor(v)}
        a = self.a = L().GemmArgs()
        a.A, a.lda, a.B, a.ldb = p(d["A"]), c.K, p(d["B"]), c.K
        a.M, a.N, a.K, a.epi, a.ldc = c.M, c.N, c.K, c.epi, c.ldc
        odt = G.out_dtype(c.epi, "C", dt)
        self.C_full, self.C = _guarded(c.M, c.N, c.ldc, odt, c.batch)
        a.C = p(self.C_full)
        if c.batch > 1:
            a.batch, a.strideA, a.strideB, a.strideC = c.batch, c.M * c.K, c.N * c.K, (c.M + GUARD) * c.ldc
        if c.bias:
            a.bias = p(d["bias"])
        if c.epi in (S.GELU, S.GELU_DG):
            self.C2_full, self.C2 = _guarded(c.M, c.N, c.ldc, G.out_dtype(c.epi, "C2", dt))
            a.C2 = p(self.C2_full)
        if "aux" in d:   # (read with C's ldc)
            self.aux = torch.zeros(c.M, c.ldc, dtype=d["aux"].dtype, device=DEV)
            self.aux[:, :c.N] = d["aux"]
            a.aux = p(self.aux)
        if c.epi == S.RESID:
            a.rowscale, a.rows_per_sample = p(d["rowscale"]), c.rps
        if c.Rp:
            a.Rp, a.B2 = c.Rp, p(d["B2"])
            if c.inside:
                self.ldt = (c.M + 31) // 32 * 32 + 32           # 32 sentinel columns beyond roundup32(M)
                self.T_full, self.T = _guarded(c.M, c.Rp, c.Rp, dt)
                self.Tt = sentinel((c.Rp + 1, self.ldt), dt)
                a.Ut, a.T_out, a.Tt_out, a.ldt, a.Ut_rank = p(d["Ut"]), p(self.T_full), p(self.Tt), self.ldt, (c.rank if c.stated else 0)
            else:
                a.A2 = p(d["A2"])
        if c.b3:
            a.B3 = p(d["B3"])
        if c.scratch:
            self.scratch = torch.empty(int(self.lib.cara_gemm_scratch_bytes()), dtype=torch.uint8, device=DEV)
            a.scratch, a.scratch_bytes = p(self.scratch), self.scratch.numel()
        self.er = c.er and riders
        self.dv = c.dv is not None and riders
        if self.er or self.dv:
            a.er_Tt, a.er_ldg, a.er_colsum = p(d["Tt"]), d["Tt"].shape[1], 1 if (c.er or c.dv) else 0
            a.er_slabs_v = C.c_void_p(16)   # (any non-NULL value for the queries)
            if self.er:
                a.er_Gt, a.er_h = p(d["Gt"]), p(self._h_ld())
                self.chunks = int(self.lib.cara_gemm_epi_rider_chunks(C.byref(a)))
                words = int(self.lib.cara_gemm_epi_rider_scratch_bytes(self.chunks, c.N)) // 4
            else:
                self.chunks = int(self.lib.cara_gemm_dv_chunks(C.byref(a), 0))
                words = int(self.lib.cara_gemm_epi_rider_scratch_bytes(self.chunks, c.K)) // 4
            assert self.chunks > 0 and words > 0
            self.sv, self.su = sentinel((words + GUARD,), torch.float32), sentinel((words + GUARD,), torch.float32)
            self.words = words
            a.er_slabs_v = p(self.sv)
            if self.er:
                a.er_slabs_u = p(self.su)
        self.ts = c.riders if riders else None

    def _h_ld(self):
        self.h = torch.zeros(self.c.M, self.c.ldc, dtype=self.dt, device=DEV)
        self.h[:, :self.c.N] = self.d["h"]
        return self.h

    def plan(self):
        out = (C.c_int * 8)(*([-1] * 8))
        c = self.c
        rc = int(self.lib.cara_debug_gemm_plan(C.byref(self.a), c.nt if self.ts else 0, 1 if (self.ts and c.riders[2]) else 0, out))
        return rc, list(out)

    def run(self):
        c, a, lib, p, st = self.c, self.a, self.lib, L().ptr, L().stream
        if self.ts:
            Rp, rank, cs = c.riders
            d, Mts = self.d, c.Mts
            nba, nbb = int(lib.cara_tskinny_scratch_bytes(Mts, 128, Rp)) // 4, int(lib.cara_tskinny_scratch_bytes(Mts, 64, Rp)) // 4
            self.sa, self.sb = sentinel((nba + GUARD,), torch.float32), sentinel((nbb + GUARD,), torch.float32)
            self.nba, self.nbb = nba, nbb
            self.fmt = int(lib.cara_gemm_rider_slab_format(C.byref(a), Rp, rank))
            L().check(lib.cara_gemm_with_tskinny_r(C.byref(a), p(d["Xa"]), 128, p(d["Gt"]), p(self.sa), 128, p(d["Xb"]), 64, p(d["Tt"]), p(self.sb), 64,
                                                   1 if cs else 0, d["Tt"].shape[1], Mts, Rp, rank, st()), "cara_gemm_with_tskinny_r")
        else:
            L().check(lib.cara_gemm_bf16(C.byref(a), st()), "cara_gemm_bf16")
        torch.cuda.synchronize()
        return self

    def _reduce(self, slabs, K1, Rp, Rc, wave_slabs, Mred, colsum):
        p, st = L().ptr, L().stream
        D_full, cs_full = sentinel((K1 + GUARD, Rp), torch.float32), sentinel((K1 + GUARD,), torch.float32)
        tab = (L().TsReduce * 1)(L().TsReduce(p(slabs), 0, p(D_full), p(cs_full) if colsum else None, 1, Mred, K1, Rp, Rc, wave_slabs))
        L().check(self.lib.cara_tskinny_reduce_many(tab, 1, st()), "reduce")
        torch.cuda.synchronize()
        assert is_sentinel(D_full[K1:]) and is_sentinel(cs_full[K1:] if colsum else cs_full)
        return D_full[:K1], cs_full[:K1]

    def outputs(self):
        """the outputs as host tensors by the model's names, after checking every sentinel"""
        c = self.c
        got = {"C": self.C.cpu()}
        assert _intact(self.C_full, c.M, c.N), "C: written beyond M rows or N columns"
        if hasattr(self, "C2"):
            got["C2"] = self.C2.cpu()
            assert _intact(self.C2_full, c.M, c.N), "C2: written beyond M rows or N columns"
        if c.inside:
            m32 = (c.M + 31) // 32 * 32
            got["T"] = self.T.cpu()
            assert _intact(self.T_full, c.M, c.Rp), "T_out: written beyond M rows"
            tt = self.Tt
            assert torch.equal(tt[:c.Rp, :c.M], self.T.t()), "Tt_out is not T_out transposed"
            assert torch.count_nonzero(tt[:c.Rp, c.M:m32].view(torch.int16)) == 0 and is_sentinel(tt[:c.Rp, m32:]) and is_sentinel(tt[c.Rp:])
            assert torch.count_nonzero(self.T[:, c.rank:].view(torch.int16)) == 0, "T_out beyond the rank"
        if self.ts:
            Rp, rank, cs = c.riders
            Rc = 16 if c.nt == 1 else 0
            assert is_sentinel(self.sa[self.nba:]) and is_sentinel(self.sb[self.nbb:])
            got["Da"], _ = self._reduce(self.sa, 128, Rp, Rc, self.fmt, c.Mts, False)
            got["Db"], csv = self._reduce(self.sb, 64, Rp, Rc, self.fmt, c.Mts, cs)
            assert torch.count_nonzero(got["Da"][:, rank:]) == 0 and torch.count_nonzero(got["Db"][:, rank:]) == 0
            got["Da"], got["Db"], got["cs"] = got["Da"].cpu(), got["Db"].cpu(), csv.cpu()
        if self.er or self.dv:
            assert is_sentinel(self.sv[self.words:]) and is_sentinel(self.su[self.words:] if self.er else self.su)
        return got


def _with_setters(c, operands, fn):
    """fn() under the case's debug setters, which are put back whatever happens"""
    lib = L().lib(operands)
    assert lib.cara_debug_set_gemm8(c.gemm8) == 0 and lib.cara_debug_set_gemm8_helpers(c.helpers) == 0
    try:
        return fn()
    finally:
        assert lib.cara_debug_set_gemm8(-1) == 0 and lib.cara_debug_set_gemm8_helpers(-1) == 0


def _assert_plan(c, launch):
    rc, out = launch.plan()
    want = [c.family, c.rows, c.block, c.nt, c.flags]
    assert rc == 0 and [out[0], out[1], out[3], out[5], out[6]] == want, f"{c.name}: plan {out} (status {rc}), written for {want}"
    return out


def _other_order(c, operands, o):
    """the host's fp32 restatement in another order: the yardstick of the aggregate rule, computed once per case and build"""
    key = (c.name, operands)
    if key not in _other:
        need = c.epi in (S.F32, S.RESID) or c.riders
        _other[key] = S.restate(c, o, S.DTYPES[operands]) if need else None
    return _other[key]


def _check(c, o, dt, got, other):
    print(f"\n{c.name} {dt}")
    res = S.holds(c, o, dt, got, other, quiet=False)
    for name, (ok, ratio, used) in res.items():
        assert ok, f"{c.name} {name}: outside its rule (worst/bound {ratio:.3f}, share / aggregate {used:.4f})"
    return res


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("c", S.CASES, ids=repr)
def test_gemm_case(c, operands):
    """One case: plan, launch, every output under its rule, every guard; with riders also C bitwise the launch without them
    (g32_epilogue_riders-fp16 is the case that found the rider epilogue's once-rounded product: docs/findings/gemm_contract.md
    section 4, item 2)."""
    dt = L().act_dtype(operands)
    o = S.operands(c, dt)

    def go():
        launch = Launch(c, o, operands)
        _assert_plan(c, launch)
        got = launch.run().outputs()
        _check(c, o, dt, got, _other_order(c, operands, o))
        if c.riders or c.er or c.dv is not None:
            # the header's promise: C (and T) bitwise the same launch without riders; then the products that rode
            plain = Launch(c, o, operands, riders=False)
            assert plain.plan()[0] == 0
            ref = plain.run().outputs()
            for name in ("C", "T"):
                assert name not in ref or torch.equal(ref[name], got[name]), f"{name} differs from the launch without riders"
        if c.er or c.dv is not None:
            Cdev = launch.C
            if c.er:
                Dv, cs = launch._reduce(launch.sv, c.N, 32, 16, launch.chunks, c.M, True)
                Du, _ = launch._reduce(launch.su, c.N, 32, 16, launch.chunks, c.M, False)
                k = G.kappa_ts_form("er", c.M, rows=c.rows, slabs=launch.chunks)
                mv, mu = G.rider_products(Cdev, o["Tt"], c.M, k), G.rider_products(o["h"], o["Gt"], c.M, k)
                (ov, oc), (ou, _) = S.restate_rider(Cdev.cpu(), o["Tt"], c.M), S.restate_rider(o["h"], o["Gt"], c.M)
                pairs = (("dVs", Dv[:, :16], mv["D"], ov), ("dc", cs, mv["colsum"], oc), ("dU", Du[:, :16], mu["D"], ou))
                assert torch.count_nonzero(Dv[:, 16:]) == 0 and torch.count_nonzero(Du[:, 16:]) == 0
            else:
                Dv, cs = launch._reduce(launch.sv, c.K, 32, 16, launch.chunks, c.M, bool(c.dv))
                mv = G.rider_products(o["A"], o["Tt"], c.M, G.kappa_ts_form("dv", c.M, slabs=-(-c.M // 160)))
                ov, oc = S.restate_rider(o["A"], o["Tt"], c.M)
                pairs = (("dVs", Dv[:, :16], mv["D"], ov),) + ((("dc", cs, mv["colsum"], oc),) if c.dv else ())
                assert torch.count_nonzero(Dv[:, 16:]) == 0
            # (fp32 sums over the rows: elementwise, and the aggregate rule against the host's other order of the same sums)
            for name, dev, (v, d), other in pairs:
                v, d = (v[:, :16], d[:, :16]) if v.dim() == 2 else (v, d)
                ok, ratio, agg = S.check_32(name, dev.cpu(), (v, d), other)
                assert ok, f"{c.name} {name}: worst/bound {ratio:.3f}, aggregate {agg:.2f}"
    _with_setters(c, operands, go)


def test_case_list_reaches_every_kernel_through_the_plan():
    """Coverage over the case list, asserted through the plan (host arithmetic only, bf16 build): families 1 to 6, tile rows 16 / 128 /
    160 / 256, helper waves, DV, epilogue riders, both adapter forms, two B operands and nt in {1, 2, 4}"""
    seen = []
    for c in S.CASES:
        o = S.operands(c, torch.bfloat16)
        seen.append(_with_setters(c, "bf16", lambda: _assert_plan(c, Launch(c, o, "bf16"))))
    assert {s[0] for s in seen} == {1, 2, 3, 4, 5, 6}
    assert {s[1] for s in seen} == {16, 128, 160, 256}
    assert {s[5] for s in seen} == {0, 1, 2, 4}
    assert {s[3] for s in seen} == {256, 512, 768}
    for flag in (S.F_COLSUM, S.F_ER, S.F_DV, S.F_TWOB, S.F_HALFT, S.F_RP64, S.F_HELPERS):
        assert any(s[6] & flag for s in seen), f"no case with plan flag {flag}"
    assert any(s[0] == G.FAM_G32 and s[7] == 8 for s in seen) and any(s[0] == G.FAM_G32 and s[7] == 1 for s in seen)   # supertiles on / off


@pytest.mark.parametrize("operands", OPERANDS)
def test_more_tiles_than_compute_units_with_a_ragged_last_round(operands):
    """three tile rows x enough column tiles for CUs + 37 tiles of 128 x 128 (the last column tile 100 wide), K = 128"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles_n = (cus + 37 + 2) // 3
    c = S.Case("many_tiles", S.G32, 128, 256, 300, 128 * tiles_n - 28, 128, S.B16)
    dt = L().act_dtype(operands)
    o = S.operands(c, dt)
    launch = Launch(c, o, operands)
    out = _assert_plan(c, launch)
    assert out[2] == 3 * tiles_n > cus
    _check(c, o, dt, launch.run().outputs(), None)


ISOLATION = ["g32_m257_resid", "ft_rank16_unstated", "batched3_bf16", "few_m17_gelu", "tile8_inside_gelu", "tile8_256_plain"]


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("name", ISOLATION)
def test_rows_of_a_and_b_reach_only_their_own_outputs(name, operands):
    """other finite values in row i of A change row i of C, C2 and T only; in row j of B column j only: every other bit stays"""
    c = next(x for x in S.CASES if x.name == name)
    dt = L().act_dtype(operands)
    o = S.operands(c, dt)
    i, j = c.M // 2, c.N // 3

    def go():
        first = Launch(c, o, operands)
        _assert_plan(c, first)
        base = first.run().outputs()
        for key, idx in (("A", i), ("B", j)):
            o2 = dict(o)
            t = o[key].clone()
            new = (torch.randn(t.shape[-1], generator=torch.Generator().manual_seed(idx)) * 0.7 - 0.2).to(dt)
            if c.batch > 1:
                t[:, idx] = new
            else:
                t[idx] = new
            o2[key] = t
            got = Launch(c, o2, operands).run().outputs()
            for nm, ref in base.items():
                if nm == "T":
                    keep = [r for r in range(c.M) if r != i] if key == "A" else list(range(c.M))
                    assert torch.equal(ref[keep], got[nm][keep]), f"T: a row other than {i} changed with {key}"
                    continue
                a, b = ref.clone().view(torch.int16 if ref.element_size() == 2 else torch.int32), got[nm].view(torch.int16 if ref.element_size() == 2 else torch.int32)
                diff = a != b
                if key == "A":
                    diff[..., i, :] = False
                else:
                    diff[..., :, j] = False
                assert not diff.any(), f"{nm}: {int(diff.sum())} elements outside {'row' if key == 'A' else 'column'} {idx} changed with {key}"
            changed = got["C"][..., i, :] if key == "A" else got["C"][..., :, j]
            same = base["C"][..., i, :] if key == "A" else base["C"][..., :, j]
            assert not torch.equal(changed, same)
    _with_setters(c, operands, go)


def _panels(X):
    M, Kc = X.shape
    return X.view(M, Kc // 32, 32).permute(1, 0, 2).contiguous()


def _layout_plans(Lm, operands, A, B, B3, bias, M, N, K):
    """the plans the layout forms were written for: the 128-row tile of FAM_G32, 256 threads, no riders; B3 alone sets a flag"""
    p = Lm.ptr
    for form in ("rows", "Bp", "a_panels", "c_panels", "B3"):
        a = Lm.GemmArgs()
        a.A, a.lda, a.B, a.ldb, a.C, a.ldc = p(A), K, p(B), K, p(A), N   # (C is not written: the plan reads the arguments only)
        a.M, a.N, a.K, a.epi, a.bias = M, N, K, Lm.EPI_BF16, p(bias)
        if form == "Bp":
            a.Bp = p(B)
        elif form == "a_panels":
            a.a_panels = a.lda = M + 3
        elif form == "c_panels":
            a.c_panels = M + 3
        elif form == "B3":
            a.B3 = p(B3)
        out = (C.c_int * 8)(*([-1] * 8))
        rc = int(Lm.lib(operands).cara_debug_gemm_plan(C.byref(a), 0, 0, out))
        want = [G.FAM_G32, 128, 256, 0, S.F_TWOB if form == "B3" else 0]
        assert rc == 0 and [out[0], out[1], out[3], out[5], out[6]] == want, f"{form}: plan {list(out)} (status {rc}), written for {want}"


@pytest.mark.parametrize("operands", OPERANDS)
def test_layout_forms_are_bitwise_their_row_major_forms(operands):
    """Bp, a_panels, c_panels and B3 at M = 129 (the smallest M the panel layouts take): the K-panel-major image of B (under
    _lib.using: pack_b_panels in the build's type), of A and of C give the row-major launch's bits; the two-B-operand launch gives
    the bits of ONE-operand launch over the 32-column steps of (A, B) and (A, B3) interleaved -- the same chain of MFMA steps"""
    Lm = L()
    dt = Lm.act_dtype(operands)
    M, N, K = 129, 160, 128
    g = torch.Generator().manual_seed(11)
    A, B, B3 = (torch.randn(s, K, generator=g).mul(sc).to(dt).to(DEV) for s, sc in ((M, 1.0), (N, 0.05), (N, 1e-4)))
    bias = torch.randn(N, generator=g).to(DEV)
    with Lm.using(operands):
        assert Lm.act_dtype() == dt
        _layout_plans(Lm, operands, A, B, B3, bias, M, N, K)
        ref = Lm.gemm(A, B, sentinel((M, N), dt), epi=Lm.EPI_BF16, bias=bias)
        Bp = Lm.pack_b_panels(B)
        assert Bp.dtype == dt and torch.equal(Bp, _panels(B))
        assert torch.equal(Lm.gemm(A, B, sentinel((M, N), dt), epi=Lm.EPI_BF16, bias=bias, Bp=Bp), ref)
        P = M + 3
        Ap = sentinel((K // 32, P, 32), dt)
        Ap[:, :M] = _panels(A)
        assert torch.equal(Lm.gemm(Ap, B, sentinel((M, N), dt), epi=Lm.EPI_BF16, bias=bias, M=M, K=K, a_panels=P), ref)
        Cp = sentinel((N // 32, P, 32), dt)
        Lm.gemm(A, B, Cp, epi=Lm.EPI_BF16, bias=bias, c_panels=P, ldc=N)
        assert torch.equal(Cp[:, :M], _panels(ref)) and is_sentinel(Cp[:, M:])
        two = Lm.gemm(A, B, sentinel((M, N), dt), epi=Lm.EPI_BF16, bias=bias, B3=B3)
        inter = lambda x, y: torch.stack((x.view(-1, K // 32, 32), y.view(-1, K // 32, 32)), 2).reshape(-1, 2 * K).contiguous()  # noqa: E731
        one = Lm.gemm(inter(A, A), inter(B, B3), sentinel((M, N), dt), epi=Lm.EPI_BF16, bias=bias)
        torch.cuda.synchronize()
        assert torch.equal(two, one) and not torch.equal(two, ref)
