"""cara_ema_update's arithmetic without a device: the numpy-fp32 restatement of tests/ema_model.py stays inside the bound derived
there against fp64 on every family of inputs, the fixed point and w == 1 hold bitwise, a fused-multiply-add variant is visible
in the bits (so the bitwise GPU check of tests/test_ema_gpu.py can see a contracted kernel), and the decay schedule of
cara_amd/ema.py is the stated one.  CPU only."""
import numpy as np
import pytest

from tests import ema_model as M

N = 20000
FAMILIES = {
    "random": lambda: M.random_pairs(N, 1),
    "random, wide": lambda: M.random_pairs(N, 2, scale=1e4),
    "p within an ulp of e": lambda: M.near_pairs(N, 3),
    "|e| >> |p|": lambda: M.lopsided_pairs(N, 4, big_e=True),
    "|p| >> |e|": lambda: M.lopsided_pairs(N, 5, big_e=False),
    "subnormals": lambda: M.subnormal_pairs(N, 6),
}


@pytest.mark.parametrize("w", M.WEIGHTS, ids=lambda w: repr(float(w)))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_restatement_stays_inside_the_derived_bound(family, w):
    e, p = FAMILIES[family]()
    if family == "subnormals":
        assert np.all(np.abs(e) < 2.0 ** -126) and np.all(np.abs(p) < 2.0 ** -126) and np.all(e != 0) and np.all(p != 0)
    got = M.update_f32(e, p, w).astype(np.float64)
    err, lim = np.abs(got - M.exact64(e, p, w)), M.bound(e, p, w)
    assert np.all(np.isfinite(got))
    worst = float(np.max(err / np.maximum(lim, 1e-300)))
    print(f"{family}, w = {float(w)!r}: worst |err| / bound {worst:.3f}")
    assert np.all(err <= lim)


def test_a_product_that_underflows_is_off_by_at_most_half_the_smallest_subnormal():
    """what the relative bound cannot cover (tests/ema_model.py): d = p - e below 2^-126 / w, any subnormal e and p"""
    r = np.random.default_rng(7)
    e = np.ldexp(r.integers(-2 ** 23 + 1, 2 ** 23, N).astype(np.float64), -149).astype(np.float32)
    p = np.ldexp(r.integers(-2 ** 23 + 1, 2 ** 23, N).astype(np.float64), -149).astype(np.float32)
    seen_outside = False
    for w in M.WEIGHTS:
        err = np.abs(M.update_f32(e, p, w).astype(np.float64) - M.exact64(e, p, w))
        seen_outside |= bool(np.any(err > M.bound(e, p, w)))
        assert np.all(err <= M.bound(e, p, w) + M.UNDERFLOW_ABS)
    assert seen_outside      # (the case exists: the absolute term is not slack)
    # the counterexample of the docstring
    assert float(M.update_f32(np.float32(0), np.float32(2.0 ** -149), np.float32(0.25))) == 0.0


def test_fixed_point_and_full_weight_hold_bitwise():
    e, p = M.random_pairs(N, 8)
    for pair in (M.near_pairs(N, 9), M.lopsided_pairs(N, 10), M.subnormal_pairs(N, 11)):
        e, p = np.concatenate([e, pair[0]]), np.concatenate([p, pair[1]])
    for w in M.WEIGHTS:
        assert np.array_equal(M.bits(M.update_f32(e, e, w)), M.bits(e)), float(w)          # p == e gives e
    assert np.array_equal(M.bits(M.update_f32(e, p, 1.0)), M.bits(p))                      # w == 1 gives p
    assert np.array_equal(M.bits(M.update_f32(e, p, 0.0)), M.bits(e))                      # w == 0 gives e
    # signed zeros: -0 stays -0 in branch 2; branch 1 gives +0 (d = +0, -0 + +0 = +0), as the header says
    nz = np.float32(-0.0)
    assert M.bits(M.update_f32(nz, nz, 0.75))[()] == M.bits(nz)[()]
    assert M.bits(M.update_f32(nz, nz, 0.25))[()] == 0


@pytest.mark.parametrize("w", M.WEIGHTS + M.EXTRA_WEIGHTS, ids=lambda w: repr(float(w)))
def test_a_fused_multiply_add_shows_in_the_bits(w):
    """on the inputs of the GPU test's kernel call: a kernel whose product and sum were contracted would not match the restatement.
    Where the factor (w in branch 1, 1 - w in branch 2) is 0, 1 or a power of two the product is exact and fusing changes nothing:
    that is every weight of WEIGHTS but the float below 0.5, which is why the GPU test also runs EXTRA_WEIGHTS."""
    differ = total = 0
    for e, p in M.kernel_case():
        differ += int(np.count_nonzero(M.bits(M.update_f32(e, p, w)) != M.bits(M.update_fma(e, p, w))))
        total += e.size
    print(f"w = {float(w)!r}: {differ} of {total} elements differ between the unfused and the fused update")
    factor = float(w) if w < np.float32(0.5) else float(np.float32(1.0) - w)
    if factor == 0.0 or np.frexp(factor)[0] == 0.5:
        assert differ == 0
    else:
        assert differ > 0      # (13 of 28 736 at w = 1 - 0.9998, where the product is far below e's last bit; a tenth at 0.1)


def test_decay_schedule():
    from cara_amd import ema as E
    d = 0.9998
    assert E.decay_at(d, False, 0) == d and E.decay_at(d, False, 10 ** 6) == d
    assert E.decay_at(d, True, 0) == 0.1 and E.decay_at(d, True, 1) == 2.0 / 11.0 and E.decay_at(d, True, 89) == 90.0 / 99.0
    # the crossover: (1 + t) / (10 + t) reaches 0.9998 at t = 44990
    assert E.decay_at(d, True, 44989) == 44990.0 / 44999.0 < d
    assert E.decay_at(d, True, 44990) == d and E.decay_at(d, True, 44991) == d and E.decay_at(d, True, 10 ** 7) == d
    for warmup in (False, True):
        for t in (0, 1, 2, 89, 44989, 44990, 10 ** 6):
            assert E.decay_at(d, warmup, t) == M.decay_at(d, warmup, t)
            w = E.weight_at(d, warmup, t)
            assert isinstance(w, float) and np.float32(w) == M.weight_at(d, warmup, t) and float(np.float32(w)) == w
    assert E.weight_at(d, True, 0) == float(np.float32(0.9))
