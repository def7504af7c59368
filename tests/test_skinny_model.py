"""Host proof of the derived bounds of the skinny-product and dense-dW kernels (oracle/skinny_model.py), on the device cases of
tests/skinny_common.py and both operand types: an fp32 restatement in ANOTHER summation order stays inside every bound and uses at
most half of every cap (tests/tolerances.py: SKINNY_CAPS); a second restatement (8 lanes) passes the aggregate rule against the first;
the restated dispatch (xu_plan, ts_chunks, tn_kslab) takes both sides of every boundary the entry points have; and each of the twelve
slips a .. l breaks a rule on at least one case.  Tables: docs/findings/skinny_contract.md (python -m tests.test_skinny_model prints
them)."""
import pytest
import torch

from oracle import skinny_model as K
from tests import skinny_common as S
from tests import tolerances as T

OPERANDS = ["bf16", "fp16"]
_cache = {}
TS_HOST = [(M, K1, Rp, rank) for M, K1 in S.TS_MK for Rp, rank in S.ts_ranks(M, K1)]


def _xu(case, operands):
    key = ("xu", case, operands)
    if key not in _cache:
        dt = S.DTYPES[operands]
        o = S.xu_operands(*case, dt)
        _cache[key] = (o, K.xu(o["X"], o["Ut"], *case), S.restate_xu(o, *case, dt))
    return _cache[key]


def _ts(case, operands):
    key = ("ts", case, operands)
    if key not in _cache:
        dt = S.DTYPES[operands]
        M, K1, Rp, rank = case
        half = Rp == 32 and rank <= 16
        o = S.ts_operands(*case, dt)
        _cache[key] = (o, K.xtg(o["X"], o["Gt"], *case, colsum=True, half=half), S.restate_xtg(o, *case, half=half), S.restate_xtg(o, *case, lanes=8, half=half))
    return _cache[key]


def _tn(case, operands):
    key = ("tn", case, operands)
    if key not in _cache:
        dt = S.DTYPES[operands]
        M, N, Kc, ns = case
        o = S.tn_operands(M, N, Kc, dt)
        _cache[key] = (o, K.tn(o["At"], o["Bt"], M, N, Kc, ns), S.restate_tn(o, M, N, Kc, ns), S.restate_tn(o, M, N, Kc, ns, lanes=8))
    return _cache[key]


def _half_cap(used, nb_free):
    """the half-cap rule; a tensor too small to express half a cap (one element of it is more) may hold ONE neighbour case, as
    gemm_common.check_16 lets it"""
    return used <= 0.5 * T.SKINNY_CAPS["T"] or nb_free


@pytest.mark.parametrize("operands", OPERANDS)
def test_xu_other_order_is_inside_every_bound_and_half_the_cap(operands):
    dt = S.DTYPES[operands]
    for case in S.XU_CASES:
        o, model, first = _xu(case, operands)
        ok, ratio, used = S.holds_xu(first, model, dt)
        print(f"xu {case} {operands} {model['plan']['kernel']} NT{model['plan']['NT']}: worst/bound {ratio:.3f} share {used:.4f}")
        assert ok, (case, ratio, used)
        assert _half_cap(used, used * first["T"].numel() <= 1.5), (case, used)


@pytest.mark.parametrize("operands", OPERANDS)
def test_xtg_other_order_is_inside_every_bound(operands):
    for case in TS_HOST:
        o, model, first, second = _ts(case, operands)
        for which, got, oth in (("first", first, second), ("second", second, first)):
            for name, (ok, ratio, agg) in S.holds_xtg(got, model, oth).items():
                assert ok, (case, which, name, ratio, agg)


@pytest.mark.parametrize("operands", OPERANDS)
def test_tn_other_order_is_inside_every_bound(operands):
    for case in S.TN_CASES:
        o, model, first, second = _tn(case, operands)
        for which, got, oth in (("first", first, second), ("second", second, first)):
            for name, (ok, ratio, agg) in S.holds_tn(got, model, oth).items():
                assert ok, (case, which, name, ratio, agg)


def test_restated_dispatch_takes_both_sides_of_every_boundary():
    """the boundaries listed in docs/findings/skinny_contract.md section 1, ticked off against the case lists"""
    plans = {c: K.xu_plan(*c) for c in S.XU_CASES}
    kinds = {(p["kernel"], p["NT"], p["groups"], p["grid_y"]) for p in plans.values()}
    assert {("sliced", 1, 1, 1), ("sliced", 2, 1, 1), ("sliced", 2, 1, 2), ("sliced", 1, 4, 1), ("sliced", 2, 4, 1), ("sliced", 2, 4, 2), ("v1", 2, 1, 1),
            ("v1", 4, 1, 1)} <= kinds
    assert K.xu_plan(63, 768, 32, 32)["kernel"] == "v1" and K.xu_plan(64, 768, 32, 32)["kernel"] == "sliced"
    assert K.xu_plan(512, 768, 32, 32)["groups"] == 1 and K.xu_plan(513, 768, 32, 32)["groups"] == 4
    assert K.xu_plan(64, 3072, 32, 32)["waves"] == 16 and K.xu_plan(64, 3264, 32, 32)["kernel"] == "v1" and K.xu_plan(64, 224, 32, 32)["kernel"] == "v1"
    assert K.xu_plan(64, 768, 32, 16)["NT"] == 1 and K.xu_plan(64, 768, 32, 17)["NT"] == 2 and K.xu_plan(64, 768, 64, 16)["NT"] == 2
    for M in (63, 64, 65, 512, 513):
        for Kc in (192, 224, 3072, 3264):
            assert any(c[0] == M and c[1] == Kc for c in S.XU_CASES), (M, Kc)
    # the transposed products: 1 .. 4 chunks, waves with 0, 1, 2, 3 and >= 4 steps, the reduction's tails n % 4 = 1, 2, 3 and none
    assert {K.ts_chunks(M, K1) for M in S.TS_M for K1 in S.TS_K1} == {1, 2, 3, 4}
    steps = set().union(*(K.ts_wave_steps(M, K1) for M, K1 in S.TS_MK))
    assert steps == {0, 1, 2, 3}                       # (>= 4 steps: M >= 2305 at K1 <= 3264 -- tests/test_kernels_gpu.py::test_tskinny)
    assert K.ts_wave_steps(2000, 3264) == {2, 3} and 5 in K.ts_wave_steps(12608, 768)
    assert max(max(K.ts_wave_steps(M, 3264)) for M in range(1, 2305)) == 3 and 4 in K.ts_wave_steps(2305, 3264)
    assert K.ts_chunks(256, 64) == 1 and K.ts_chunks(257, 64) == 2           # the cap ceil(steps / 8)
    assert K.ts_chunks(100000, 64 * 256) == 1 and K.ts_chunks(100000, 64 * 128) == 2   # the cap ceil(256 / colblocks)
    # the dense dW: one step, a ragged only step, ragged last steps, a slab of exactly 32 rows, refused pairs
    assert K.tn_kslab(33, 2) == 32 and K.tn_kslab(32, 2) is None and K.tn_kslab(64, 3) is None and K.tn_kslab(95, 3) == 32 and K.tn_kslab(333, 3) == 128
    assert K.tn_kslab(1, 0) is None and K.tn_kslab(10 ** 7, 65536) is None


def slip_table():
    """per slip: (cases x builds it applies to, on which it breaks a rule)"""
    rows = {s: [0, 0] for s in S.SLIPS}
    for operands in OPERANDS:
        dt = S.DTYPES[operands]
        for case in S.XU_CASES:
            o, model, first = _xu(case, operands)
            for s in S.XU_SLIPS:
                if S.xu_slip_applies(*case, s):
                    rows[s][0] += 1
                    rows[s][1] += not S.holds_xu(S.restate_xu(o, *case, dt, slip=s), model, dt)[0]
        for case in TS_HOST:
            o, model, first, second = _ts(case, operands)
            half = case[2] == 32 and case[3] <= 16
            for s in S.TS_SLIPS:
                if S.ts_slip_applies(*case, s, half=half):
                    rows[s][0] += 1
                    rows[s][1] += not all(r[0] for r in S.holds_xtg(S.restate_xtg(o, *case, slip=s, half=half), model, first).values())
        for case in S.TN_CASES:
            o, model, first, second = _tn(case, operands)
            for s in S.TN_SLIPS:
                if S.tn_slip_applies(*case, s):
                    rows[s][0] += 1
                    rows[s][1] += not all(r[0] for r in S.holds_tn(S.restate_tn(o, *case, slip=s), model, first).values())
    return rows


def test_every_slip_breaks_a_rule_on_some_case():
    rows = slip_table()
    print("\nslip: cases x builds it applies to / on which it breaks a rule")
    for s, (n, broke) in rows.items():
        print(f"  {s} {S.SLIPS[s]:60s} {n:4d} {broke:4d}")
    for s, (n, broke) in rows.items():
        assert n > 0 and broke > 0, f"slip {s}: applies to {n}, breaks none"


def host_shares():
    """the restatement's worst ratio and largest neighbour share / aggregate per output and build: what SKINNY_CAPS is chosen from"""
    worst = {}

    def put(k, ratio, used):
        w = worst.get(k, (0.0, 0.0))
        worst[k] = (max(w[0], ratio), max(w[1], used))
    for operands in OPERANDS:
        dt = S.DTYPES[operands]
        for case in S.XU_CASES:
            o, model, first = _xu(case, operands)
            ok, ratio, used = S.holds_xu(first, model, dt)
            put(("T", operands), ratio, used)
        for case in TS_HOST:
            o, model, first, second = _ts(case, operands)
            for name, (ok, ratio, agg) in S.holds_xtg(first, model, second).items():
                put((name, operands), ratio, agg)
        for case in S.TN_CASES:
            o, model, first, second = _tn(case, operands)
            for name, (ok, ratio, agg) in S.holds_tn(first, model, second).items():
                put(("tn", operands), ratio, agg)
    return worst


if __name__ == "__main__":
    print(f"{len(S.XU_CASES)} xu cases, {len(TS_HOST)} transposed, {len(S.TN_CASES)} tn")
    for (k, operands), (ratio, used) in sorted(host_shares().items()):
        print(f"{k:18s} {operands}: worst/bound {ratio:.3f}  share or aggregate {used:.4f}")
    for s, row in slip_table().items():
        print(s, S.SLIPS[s], row)
