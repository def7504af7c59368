"""Host proof of the GEMM family's derived bounds (oracle/gemm_model.py), on the small device cases of tests/gemm_common.py and
both operand types: an fp32 restatement in ANOTHER summation order stays inside every bound and uses at most half of every cap
(tests/tolerances.py: GEMM_CAPS); a second restatement with K split eight ways passes the aggregate rule against the first; the
restatement of gelu_erf / gelu_erf_grad lies within its stated distance of the true erf GELU; and each of twelve plausible slips
breaks a rule on at least one case.  Tables: docs/findings/gemm_contract.md (python -m tests.test_gemm_model prints them)."""
import math

import pytest
import torch

from oracle import gemm_model as G
from tests import gemm_common as S
from tests import tolerances as T

OPERANDS = ["bf16", "fp16"]
_cache = {}


def _case(c, operands):
    """operands, the restatement (32 lanes) and the second one (8 lanes) of a case: computed once, shared, left unchanged"""
    key = (c.name, operands)
    if key not in _cache:
        dt = S.DTYPES[operands]
        o = S.operands(c, dt)
        _cache[key] = (o, S.restate(c, o, dt), S.restate(c, o, dt, lanes=8))
    return _cache[key]


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("c", S.HOST_CASES, ids=repr)
def test_other_order_restatement_is_inside_every_bound_and_half_of_every_cap(c, operands):
    dt = S.DTYPES[operands]
    o, first, second = _case(c, operands)
    print(f"\n{c.name} {operands}")
    for name, (ok, ratio, used) in S.holds(c, o, dt, first, second, quiet=False).items():
        assert ok, f"{c.name} {name}: outside its rule (worst/bound {ratio:.3f}, {used})"
        if S.is16(c, name.split("@")[0]) and name not in ("Da", "Db", "cs"):
            assert used <= 0.5 * T.GEMM_CAPS[S.kind(c, name.split("@")[0])], (c.name, name, used)


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("c", [c for c in S.HOST_CASES if c.epi in (S.F32, S.RESID) or c.riders], ids=repr)
def test_second_restatement_passes_the_aggregate_rule(c, operands):
    """the fp32 outputs of the restatement with K split eight ways, held as the device is: elementwise and, per row family, within
    BWD_VS_MODEL_ORDER of the first restatement's RMS distance from the float64 value"""
    dt = S.DTYPES[operands]
    o, first, second = _case(c, operands)
    for name, (ok, ratio, agg) in S.holds(c, o, dt, second, first).items():
        assert ok, f"{c.name} {name}: worst/bound {ratio:.3f}, aggregate {agg}"


def test_gelu_restatement_against_the_true_erf_gelu():
    """u in [-12, 12] with +-0 and the points where fmaxf(u, 0) switches; the term is absolute, and on the negative tail it is larger
    than the value it holds"""
    tiny = 2.0 ** -126
    u = torch.cat((torch.linspace(-12, 12, 48001, dtype=torch.float64), torch.tensor([0.0, -0.0, tiny, -tiny, 2.0 ** -149, -2.0 ** -149], dtype=torch.float64)))
    true, true_g, b, b_g = G.gelu_vs_true(u)
    g, gp = G.gelu(u)[0], G.gelu_grad(u)[0]
    r, r_g = float(((g - true).abs() / b).max()), float(((gp - true_g).abs() / b_g).max())
    print(f"\ngelu restatement vs true erf GELU: worst/bound {r:.3f}, derivative {r_g:.3f}; max abs {float((g - true).abs().max()):.3e} / {float((gp - true_g).abs().max()):.3e}")
    assert r <= 1.0 and r_g <= 1.0
    assert float(g[u == 0].abs().max()) == 0.0 and float((gp[u == 0] - 0.5).abs().max()) <= b_g[u == 0].max()
    i = int((u + 5).abs().argmin())
    assert b[i] > true[i].abs()      # gelu(-5) = -1.4e-6 is held by the absolute term alone
    # the fp32 evaluation of the same formulas is within the counted roundings of the float64 restatement
    u32 = u.float()
    for fn, grad in ((G.gelu, False), (G.gelu_grad, True)):
        v, d = fn(u32)
        assert bool(((S.gelu_f32(u32, grad=grad).double() - v).abs() <= d).all())


def _old_bar(c, name, got, ref):
    """what the corresponding test of tests/test_kernels_gpu.py asked: 2^-8 relative + 1e-3 absolute on a 16-bit output, 1e-4 relative
    + 1e-3 sqrt(K / 64) + 2e-3 absolute on an fp32 one (riders: 1e-3, 2e-2) -> True if `got` FAILS it"""
    err = (got.double() - ref).abs()
    if name in ("Da", "Db", "cs"):
        return bool((err > 2e-2 + 1e-3 * ref.abs()).any())
    if S.is16(c, name):
        return bool((err > 1e-3 + 2.0 ** -8 * ref.abs()).any())
    return bool((err > 1e-3 * math.sqrt(c.K / 64) + 2e-3 + 1e-4 * ref.abs()).any())


def slip_table(operands_list=OPERANDS):
    """per slip: cases it applies to, cases on which it breaks a rule, and whether the OLD bar catches it on the Gaussian rows of
    those cases (the one family the older tests draw)"""
    rows = {}
    for slip in S.SLIPS:
        n = broke = old = 0
        for c in S.HOST_CASES:
            if not S.slip_applies(c, slip):
                continue
            for operands in operands_list:
                dt = S.DTYPES[operands]
                o, first, _ = _case(c, operands)
                bad = S.restate(c, o, dt, slip=slip)
                res = S.holds(c, o, dt, bad, first)
                n += 1
                broke += any(not ok for ok, _, _ in res.values())
                gauss = [i for i, f in enumerate(o["fam"]) if f == 0]
                md = S.model(c, o, dt, T_dev=bad.get("T"))
                caught = False
                for name, (v, _) in md.items():
                    if name == "T" or c.batch > 1 or not gauss:
                        continue
                    ref = G.round16(v, dt).double() if name == "C2" and c.epi == S.GELU else v
                    caught |= _old_bar(c, name, bad[name][gauss], ref[gauss])
                if c.riders:
                    for name, (v, _) in S.model_riders(c, o).items():
                        caught |= _old_bar(c, name, bad[name], v)
                old += caught
        rows[slip] = (n, broke, old)
    return rows


def test_every_slip_breaks_a_rule_on_some_device_shape():
    rows = slip_table()
    print("\nslip: cases x builds / break a rule / fail the old bar")
    for slip, (n, broke, old) in rows.items():
        print(f"  {slip:22s} {n:3d} {broke:3d} {old:3d}")
    for slip, (n, broke, old) in rows.items():
        assert n > 0 and broke > 0, f"{slip}: applies to {n} cases, breaks none"


def host_shares():
    """the restatement's largest neighbour share per output kind and build: what GEMM_CAPS is chosen from"""
    worst = {}
    for operands in OPERANDS:
        dt = S.DTYPES[operands]
        for c in S.HOST_CASES:
            o, first, second = _case(c, operands)
            for name, (ok, ratio, used) in S.holds(c, o, dt, first, second).items():
                base = name.split("@")[0]
                if base in ("Da", "Db", "cs"):
                    k = ("rider_" + base, operands)
                    worst[k] = max(worst.get(k, (0, 0)), (ratio, used))
                    continue
                k = (S.kind(c, base) if S.is16(c, base) else "fp32", operands)
                w = worst.get(k, (0.0, 0.0))
                worst[k] = (max(w[0], ratio), max(w[1], used))
    return worst


if __name__ == "__main__":
    for (k, operands), (ratio, used) in sorted(host_shares().items()):
        print(f"{k:10s} {operands}: worst/bound {ratio:.3f}  share or aggregate {used:.4f}")
    for slip, row in slip_table().items():
        print(slip, row)
