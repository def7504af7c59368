"""Host proof of the derived bounds of oracle/exact_modes_model.py (dropout_exact.hip, dense_delta.hip), on the device cases of
tests/exact_modes_common.py and both operand types: an fp32 restatement of every output in ANOTHER order stays inside every bound,
uses at most half of every cap (tests/tolerances.py: EXACT_CAPS) and satisfies the aggregate rule against a second, different
restatement; each slip of exact_modes_common.SLIPS leaves a bound on at least one case.  Tables: docs/findings/exact_modes_contract.md
(python -m tests.test_exact_modes_model prints them)."""
import numpy as np
import pytest
import torch

from cara_amd.dropout import keep_mask
from oracle import exact_modes_model as E
from tests import exact_modes_common as S
from tests import tolerances as T

OPERANDS = ["bf16", "fp16"]
HOST_DD = S.DD_GEOMS[:4]          # the DD_MAXLK geometry's model and restatement run once, in the device test
_cache = {}


def cached(key, make):
    """models and inputs are computed once, shared by the host and the device test, and left unchanged"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def linear_inputs(shape, Rp, family, operands):
    return cached(("lin", shape, Rp, family, operands), lambda: S.draw_linear(*shape, Rp, family, S.DTYPES[operands]))


def merge_model(shape, Rp, run, operands, with_w):
    p, seed, lin, family = run[:4]
    W, Um, Vs = linear_inputs(shape, Rp, family, operands)
    return cached(("merge", shape, Rp, run, operands, with_w), lambda: E.merge(W if with_w else None, Um, Vs, p, seed, lin))


def contract_inputs(shape, run):
    return cached(("slabs", shape, run[3], run[4]), lambda: S.draw_slabs(*shape, run[4], run[3]))


def contract_model(shape, Rp, run, operands):
    p, seed, lin, family = run[:4]
    _, Um, Vs = linear_inputs(shape, Rp, family, operands)
    return cached(("contract", shape, Rp, run, operands), lambda: E.contract(contract_inputs(shape, run), Um, Vs, p, seed, lin))


def colsum_model(case, operands):
    M, N, ld = case
    X = cached(("X", case, operands), lambda: S.draw_colsum(M, N, S.DTYPES[operands]))
    return X, cached(("colsum", case, operands), lambda: E.colsum(X, M, N))


def dd_inputs(geom, early):
    return cached(("dd_in", geom, early), lambda: S.draw_dd(geom, early))


def dd_models(geom, early):
    A1, A2, R1, dD = dd_inputs(geom, early)
    return cached(("dd", geom, early), lambda: (E.dd_materialize(A1, A2, R1, S.S, geom[1]), E.dd_grad(A1, A2, R1, dD, S.S, geom[1])))


def contract_rows(shape, family):
    return {k: S.outlier_rows(k, shape=shape, family=family) for k in ("dVs", "dU")}


def dd_rows(geom):
    return {k: S.outlier_rows(k, geom=geom) for k in ("A2", "A1", "R1")}


# --- the mask ---------------------------------------------------------------------------------------------------------------
def test_threshold_is_the_fp32_p():
    """(float)0.3 * 2^24 = 5033165 exactly; the double 0.3 * 2^24 floors to 5033164: keep_mask's and the model's threshold is the former"""
    assert E.mask_params(0.3)[0] == 5033165 and int(0.3 * 16777216.0) == 5033164
    h = np.array([5033164 << 8, 5033165 << 8], dtype=np.uint32)
    assert list((h >> np.uint32(8)) >= np.uint32(E.mask_params(0.3)[0])) == [False, True]
    for p in S.PS:
        for seed, lin in zip(S.SEEDS, S.LINS):
            assert np.array_equal(keep_mask(65, 63, p, seed, lin), E.keep(65, 63, p, seed, lin).numpy())
    assert E.mask_params(0.0) == (0, 1.0) and abs(E.mask_params(0.999)[1] - 1000.0) < 0.02
    assert all(E.mask_params(p) is None for p in (1.0, -0.1, float("nan")))


def test_colsum_policy_cases():
    assert [E.colsum_chunks(M, N) for M, N, _ in S.COLSUM] == [1, 1, 10, 16, 16, 32]
    assert [E.colsum_empty_chunks(M, N) for M, N, _ in S.COLSUM] == [0, 0, 0, 0, 0, 1] and S.COLSUM[-1] == S.COLSUM_EMPTY


def test_sum_slabs_order():
    x = torch.randn(5, 7, generator=torch.Generator().manual_seed(1))
    assert torch.equal(E.sum_slabs(x, 5), ((x[0] + x[2]) + x[4]) + (x[1] + x[3]))
    assert torch.equal(E.sum_slabs(x, 1), x[0]) and torch.equal(E.sum_slabs(x, 2), x[0] + x[1])


# --- the restatement inside every bound ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("Rp", S.RPS)
@pytest.mark.parametrize("shape", S.SHAPES, ids=S.sid)
def test_linear_restatement_is_inside_every_bound(shape, Rp, operands):
    dt = S.DTYPES[operands]
    for run in S.runs():
        p, seed, lin, family, nslab, gap = run
        W, Um, Vs = linear_inputs(shape, Rp, family, operands)
        for with_w in (True, False):
            got = S.restate_merge(W, Um, Vs, p, seed, lin, dt, with_w)
            ok, ratio, used = S.holds_merge("merge", got, merge_model(shape, Rp, run, operands, with_w), dt, with_w, frac=0.5)
            assert ok, f"merge {run} W={with_w}: worst/bound {ratio:.3f}, share {used}"
        slabs = contract_inputs(shape, run)
        a, b = (S.restate_contract(slabs, Um, Vs, p, seed, lin, order=o) for o in "AB")
        for name, (ok, ratio, agg) in S.holds_f32(contract_model(shape, Rp, run, operands), a, b, contract_rows(shape, family)).items():
            assert ok, f"{name} {run}: worst/bound {ratio:.3f}, aggregate {agg:.2f}"


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("case", S.COLSUM, ids=S.sid)
def test_colsum_restatement_is_inside_its_bound(case, operands):
    M, N, ld = case
    X, (v, d, chunks) = colsum_model(case, operands)
    assert chunks == E.colsum_chunks(M, N)
    ok, ratio, agg = S.holds_f32({"colsum": (v, d)}, {"colsum": S.restate_colsum(X, M, N)}, {"colsum": S.restate_colsum(X, M, N, order="B")})["colsum"]
    assert ok, f"worst/bound {ratio:.3f}, aggregate {agg:.2f}"


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("geom", HOST_DD, ids=S.sid)
def test_dense_delta_restatement_is_inside_every_bound(geom, operands):
    dt = S.DTYPES[operands]
    for early in (False, True):
        A1, A2, R1, dD = dd_inputs(geom, early)
        mat, grad = dd_models(geom, early)
        ok, ratio, used = S.holds_dd_materialize(S.restate_dd_materialize(A1, A2, R1, S.S, geom[1], dt), mat, dt, frac=0.5)
        assert ok, f"Dm early={early}: worst/bound {ratio:.3f}, share {used}"
        if operands == "bf16":      # (the gradients are fp32 in, fp32 out: the same in both builds)
            a, b = (S.restate_dd_grad(A1, A2, R1, dD, S.S, geom[1], order=o) for o in "AB")
            for name, (ok, ratio, agg) in S.holds_f32(grad, a, b, dd_rows(geom)).items():
                assert ok, f"d{name} early={early}: worst/bound {ratio:.3f}, aggregate {agg:.2f}"


# --- the slips --------------------------------------------------------------------------------------------------------------
def _slip_cases(kernel):
    if kernel in ("merge", "contract"):
        return [(shape, Rp, run) for shape in S.SHAPES for Rp in S.RPS for run in S.runs()]
    return S.COLSUM if kernel == "colsum" else [(g, e) for g in HOST_DD for e in (False, True)]


def _slip_breaks(kernel, case, slip, operands="bf16"):
    dt = S.DTYPES[operands]
    if kernel in ("merge", "contract"):
        shape, Rp, run = case
        p, seed, lin, family = run[:4]
        W, Um, Vs = linear_inputs(shape, Rp, family, operands)
        if kernel == "merge":
            return any(not S.holds_merge("merge", S.restate_merge(W, Um, Vs, p, seed, lin, dt, w, slip=slip), merge_model(shape, Rp, run, operands, w), dt, w)[0]
                       for w in (True, False))
        got = S.restate_contract(contract_inputs(shape, run), Um, Vs, p, seed, lin, slip=slip)
        return any(not r[0] for r in S.holds_f32(contract_model(shape, Rp, run, operands), got, None).values())
    if kernel == "colsum":
        X, (v, d, _) = colsum_model(case, operands)
        return not S.holds_f32({"colsum": (v, d)}, {"colsum": S.restate_colsum(X, case[0], case[1], slip=slip)}, None)["colsum"][0]
    geom, early = case
    A1, A2, R1, dD = dd_inputs(geom, early)
    mat, grad = dd_models(geom, early)
    if kernel == "dd_materialize":
        return not S.holds_dd_materialize(S.restate_dd_materialize(A1, A2, R1, S.S, geom[1], dt, slip=slip), mat, dt)[0]
    return any(not r[0] for r in S.holds_f32(grad, S.restate_dd_grad(A1, A2, R1, dD, S.S, geom[1], slip=slip), None).values())


def slip_table():
    """per slip: cases evaluated / cases on which it leaves a bound"""
    rows = {}
    for slip in S.SLIPS:
        n = broke = 0
        for kernel in S.SLIP_KERNELS[slip]:
            for case in _slip_cases(kernel):
                n += 1
                broke += bool(_slip_breaks(kernel, case, slip))
        rows[slip] = (n, broke)
    return rows


def test_every_slip_leaves_a_bound_on_some_case():
    rows = cached("slips", slip_table)
    print("\nslip: cases evaluated / cases that catch it")
    for slip, (n, broke) in rows.items():
        print(f"  {slip:28s} {n:3d} {broke:3d}" + ("" if broke else "   UNCAUGHT"))
    for slip, (n, broke) in rows.items():
        assert n > 0 and broke > 0, f"{slip}: {n} cases, none catches it"


# --- the tables ---------------------------------------------------------------------------------------------------------------
def host_tables():
    """the restatement's largest neighbour share per 16-bit kind, family and build (what EXACT_CAPS is recorded from) and its worst
    worst/bound and aggregate ratio per fp32 output"""
    caps, f32 = {}, {}

    def cap(kind, family, operands, ratio, used):
        w = caps.get((kind, family, operands), (0.0, 0.0))
        caps[(kind, family, operands)] = (max(w[0], ratio), max(w[1], used))

    def put(name, res):
        w = f32.get(name, (0.0, 0.0))
        f32[name] = (max(w[0], res[1]), max(w[1], res[2]))
    for operands in OPERANDS:
        dt = S.DTYPES[operands]
        for shape in S.SHAPES:
            for Rp in S.RPS:
                for run in S.runs():
                    p, seed, lin, family = run[:4]
                    W, Um, Vs = linear_inputs(shape, Rp, family, operands)
                    for w in (True, False):
                        _, ratio, used = S.holds_merge("merge", S.restate_merge(W, Um, Vs, p, seed, lin, dt, w), merge_model(shape, Rp, run, operands, w), dt, w)
                        cap("merge_Weff" if w else "merge_Dm", family, operands, ratio, used)
                    slabs = contract_inputs(shape, run)
                    a, b = (S.restate_contract(slabs, Um, Vs, p, seed, lin, order=o) for o in "AB")
                    for name, res in S.holds_f32(contract_model(shape, Rp, run, operands), a, b, contract_rows(shape, family)).items():
                        put(name, res)
        for case in S.COLSUM:
            X, (v, d, _) = colsum_model(case, operands)
            put("colsum", S.holds_f32({"colsum": (v, d)}, {"colsum": S.restate_colsum(X, *case[:2])}, {"colsum": S.restate_colsum(X, *case[:2], order="B")})["colsum"])
        for geom in HOST_DD:
            for early in (False, True):
                A1, A2, R1, dD = dd_inputs(geom, early)
                mat, grad = dd_models(geom, early)
                _, ratio, used = S.holds_dd_materialize(S.restate_dd_materialize(A1, A2, R1, S.S, geom[1], dt), mat, dt)
                cap("dd_Dm", "early" if early else "gaussian", operands, ratio, used)
                if operands == "bf16":
                    a, b = (S.restate_dd_grad(A1, A2, R1, dD, S.S, geom[1], order=o) for o in "AB")
                    for name, res in S.holds_f32(grad, a, b, dd_rows(geom)).items():
                        put("dd_d" + name, res)
    return caps, f32


if __name__ == "__main__":
    caps, f32 = host_tables()
    print("16-bit kind, family, build: worst/bound, largest neighbour share, cap")
    for (kind, family, operands), (ratio, used) in sorted(caps.items()):
        print(f"  {kind:10s} {family:8s} {operands}: {ratio:.3f}  {used:.4f}  cap {T.EXACT_CAPS[kind]} ({'<= half' if used <= 0.5 * T.EXACT_CAPS[kind] else 'ABOVE HALF'})")
    print("fp32 output: worst/bound, aggregate ratio against the second restatement")
    for name, (ratio, agg) in sorted(f32.items()):
        print(f"  {name:8s} {ratio:.3f}  {agg:.2f}")
    print("kappa: merge", {(Rp, p, w): E.kappa_merge(Rp, p, w) for Rp in S.RPS for p in (0.0, 0.1) for w in (True, False)})
    print("kappa: contract (nslab 5, p > 0)", {sh: (E.kappa_contract(5, 0.1, -(-sh[1] // 64)), E.kappa_contract(5, 0.1, -(-sh[0] // 64))) for sh in S.SHAPES})
    print("kappa: colsum", {c: max(E.kappa_colsum(c[0], n) for n in E.colsum_chunk_chain(c[0], c[1])) for c in S.COLSUM})
    print("kappa: dense delta", {g: (E.kappa_dd_materialize(g[2]), E.kappa_dd_grad(*g)) for g in S.DD_GEOMS})
    print("slip: cases evaluated / cases that catch it")
    for slip, (n, broke) in slip_table().items():
        print(f"  {slip:28s} {n:3d} {broke:3d}" + ("" if broke else "   UNCAUGHT"))
