"""Host proof of the adapter-side kernels' derived bounds (oracle/adapter_model.py), on the device geometries of
tests/adapter_common.py and both operand types: an fp32 restatement of cara_factor_prep and cara_factor_grad_reduce(_ex) in ANOTHER
order stays inside every bound and uses at most half of the cap (tests/tolerances.py: ADAPTER_CAPS), and each of thirteen plausible
slips breaks a rule on at least one geometry.  Tables: docs/findings/adapter_contract.md (python -m tests.test_adapter_model prints
them)."""
import pytest
import torch

from oracle import adapter_model as A
from oracle import cara_oracle as O
from tests import adapter_common as S
from tests import tolerances as T

OPERANDS = ["bf16", "fp16"]
DRAWS = [False, True]   # early
_cache = {}


def inputs(geom, early):
    key = ("in", geom, early)
    if key not in _cache:
        _cache[key] = (S.draw_cp(geom, early), S.draw_bias(geom))
    return _cache[key]


def prep_model(geom, early):
    """float64 (v, d) of the pack: computed once, shared by both builds and by the device test, left unchanged"""
    key = ("prep", geom, early)
    if key not in _cache:
        cp, bias = inputs(geom, early)
        _cache[key] = A.factor_prep(cp, bias, geom, S.S)
    return _cache[key]


def grad_model(geom, early, family, loss_scale=None):
    key = ("grad", geom, early, family, loss_scale)
    if key not in _cache:
        cp, _ = inputs(geom, early)
        lg = S.draw_lg(geom, family)
        _cache[key] = (lg, A.factor_grad_reduce(cp, lg, geom, S.S, loss_scale))
    return _cache[key]


GRAD_RUNS = [(False, f) for f in S.FAMILIES] + [(True, "gaussian")]


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("geom", S.GEOMS, ids=S.gid)
def test_prep_restatement_is_inside_every_bound_and_half_of_the_cap(geom, operands):
    dt = S.DTYPES[operands]
    for early in DRAWS:
        cp, bias = inputs(geom, early)
        print(f"\n{S.gid(geom)} {operands} early={early}")
        for name, (ok, ratio, used) in S.holds_prep(geom, prep_model(geom, early), S.restate_prep(cp, bias, geom, dt), dt, quiet=False).items():
            assert ok, f"{name}: outside its rule (worst/bound {ratio:.3f}, share {used})"
            assert used is None or used <= 0.5 * T.ADAPTER_CAPS["pack"], (name, used)


@pytest.mark.parametrize("geom", S.GEOMS, ids=S.gid)
def test_grad_restatement_is_inside_every_bound(geom):
    written = set(A.kappa_grad(geom))
    assert written == set(A.cp_names(geom[5])) - ({"A1", "A2"} if geom[5] == 2 else set())
    for early, family in GRAD_RUNS:
        cp, _ = inputs(geom, early)
        lg, model = grad_model(geom, early, family)
        got = S.restate_grad(cp, lg, geom)
        assert set(got) == written
        for name, (ok, ratio) in S.holds_grad(model, got).items():
            print(f"  {S.gid(geom)} early={early} {family} {name}: worst/bound {ratio:.3f}")
            assert ok, f"{name} ({family}, early={early}): worst/bound {ratio:.3f}"
        if geom[5] == 2:
            assert float(got["R1"].abs().max()) == 0.0


@pytest.mark.parametrize("geom", S.EX_GEOMS, ids=S.gid)
def test_loss_scale_restatement(geom):
    """a power of two scales every output bitwise; 1000 stays inside the bound grown by 2u |v|"""
    cp, _ = inputs(geom, False)
    lg, _ = grad_model(geom, False, "gaussian")
    plain = S.restate_grad(cp, lg, geom)
    for k in (10, 16):
        scaled = S.restate_grad(cp, lg, geom, loss_scale=2.0 ** k)
        for name in plain:
            assert torch.equal(scaled[name], plain[name] * 2.0 ** -k), name
    _, model = grad_model(geom, False, "gaussian", 1000.0)
    for name, (ok, ratio) in S.holds_grad(model, S.restate_grad(cp, lg, geom, loss_scale=1000.0)).items():
        assert ok, f"{name}: worst/bound {ratio:.3f}"


# --- the slips --------------------------------------------------------------------------------------------------------------
def _old_inputs():
    """the inputs of tests/test_kernels_gpu.py::test_factor_prep_and_grad_reduce at rank 16: synthetic_cp, s = 0.1, Gaussian
    gradients WITH Gaussian padding columns"""
    if "old" not in _cache:
        geom = S.OLD_GEOM
        cp = {k[3:]: v for k, v in O.synthetic_cp(rank=geom[3]).items()}
        g = torch.Generator().manual_seed(9)
        lg = {k: torch.randn(*shape, generator=g) for k, shape in S.lg_shapes(geom).items()}
        bias = [torch.randn(geom[0], n, generator=g) for n in (geom[1], 4 * geom[1], geom[1])]
        _cache["old"] = (cp, lg, bias, A.factor_grad_reduce(cp, lg, geom, 0.1), A.factor_prep(cp, bias, geom, 0.1))
    return _cache["old"]


def _old_bar_fails(slip):
    """would the old test have failed this slip?  Its prep bars on layers 0, 5, 11 (U bitwise; Vs rtol 2^-7, atol 1e-8 against the
    rounded reference; Vst the transpose of Vs; biases rtol 1e-6, atol 1e-7) and its gradient bar 1e-4 (|ref| + max |ref|)"""
    geom = S.OLD_GEOM
    R = geom[3]
    cp, lg, bias, gmodel, (mats, bmodel) = _old_inputs()
    if slip == "loss_scale_not_on_R":
        return False                     # (the old test never calls the _ex entry)
    got = S.restate_grad(cp, lg, geom, slip=slip, s=0.1)
    if any(S.old_bar_fails(got[name], v) for name, (v, _) in gmodel.items()):
        return True
    pk = S.restate_prep(cp, bias, geom, torch.bfloat16, slip=slip, s=0.1)
    for l in (0, 5, 11):
        for name in A.MATS:
            ref = A.round16(mats[name][0][l], torch.bfloat16)
            g = pk[name][l, :, :R]
            if name.startswith("U_"):
                if not torch.equal(g, ref) or not torch.equal(pk[name + "_t"][l, :R], ref.t()):
                    return True
            elif not torch.allclose(g.float(), ref.float(), rtol=2 ** -7, atol=1e-8) or not torch.equal(pk[name + "_t"][l, :R].float(), g.float().t()):
                return True
    return False


def slip_table():
    """per slip: (geometry, run)s it applies to, those on which it breaks a rule, and whether the OLD test's bars catch it at the old
    test's single geometry and inputs"""
    rows = {}
    for slip in S.SLIPS:
        n = broke = 0
        for geom in S.GEOMS:
            if not S.slip_applies(geom, slip):
                continue
            n += 1
            bad = False
            if slip == "loss_scale_not_on_R":
                cp, _ = inputs(geom, False)
                lg, model = grad_model(geom, False, "gaussian", 1000.0)
                bad = any(not ok for ok, _ in S.holds_grad(model, S.restate_grad(cp, lg, geom, slip=slip, loss_scale=1000.0)).values())
            else:
                for early, family in GRAD_RUNS:
                    cp, _ = inputs(geom, early)
                    lg, model = grad_model(geom, early, family)
                    bad |= any(not ok for ok, _ in S.holds_grad(model, S.restate_grad(cp, lg, geom, slip=slip)).values())
                for early in DRAWS:
                    cp, bias = inputs(geom, early)
                    pk = S.restate_prep(cp, bias, geom, torch.bfloat16, slip=slip)
                    bad |= any(not r[0] for r in S.holds_prep(geom, prep_model(geom, early), pk, torch.bfloat16).values())
            broke += bad
        rows[slip] = (n, broke, _old_bar_fails(slip))
    return rows


def test_every_slip_breaks_a_rule_on_some_geometry():
    rows = slip_table()
    print("\nslip: geometries it applies to / breaks a rule on / fails the old bar at the old geometry")
    for slip, (n, broke, old) in rows.items():
        print(f"  {slip:28s} {n:2d} {broke:2d} {'yes' if old else 'no'}")
    for slip, (n, broke, old) in rows.items():
        assert n > 0 and broke > 0, f"{slip}: applies to {n} geometries, breaks none"


def test_unslipped_restatement_passes_the_old_bar():
    """the column of the slips table means something only if the restatement itself passes the old test"""
    assert not _old_bar_fails(None)


def host_tables():
    """the restatement's worst / bound and largest neighbour share per output and build: what ADAPTER_CAPS is recorded from"""
    prep, grad = {}, {}
    for geom in S.GEOMS:
        for operands in OPERANDS:
            dt = S.DTYPES[operands]
            for early in DRAWS:
                cp, bias = inputs(geom, early)
                for name, (ok, ratio, used) in S.holds_prep(geom, prep_model(geom, early), S.restate_prep(cp, bias, geom, dt), dt).items():
                    w = prep.get((name, operands), (0.0, 0.0, None))
                    big = used if (used is not None and used > w[1]) else w[1]
                    prep[(name, operands)] = (max(w[0], ratio), big, S.gid(geom) if big != w[1] else w[2])
        for early, family in GRAD_RUNS:
            cp, _ = inputs(geom, early)
            lg, model = grad_model(geom, early, family)
            for name, (ok, ratio) in S.holds_grad(model, S.restate_grad(cp, lg, geom)).items():
                k = A.kappa_grad(geom)[name]
                w = grad.get((name, geom[5]), (0.0, 0, 0))
                grad[(name, geom[5])] = (max(w[0], ratio), max(w[1], max(k) if isinstance(k, list) else k), 0)
    return prep, grad


if __name__ == "__main__":
    prep, grad = host_tables()
    for (name, operands), (ratio, used, where) in sorted(prep.items()):
        print(f"pack {name:10s} {operands}: worst/bound {ratio:.3f}  largest share {used:.4f} ({where})")
    for (name, order), (ratio, kmax, _) in sorted(grad.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        print(f"grad order {order} {name:6s}: worst/bound {ratio:.3f}  largest kappa {kmax}")
    for geom in S.GEOMS:
        print(S.gid(geom), A.kappa_grad(geom))
    for slip, row in slip_table().items():
        print(slip, row)
