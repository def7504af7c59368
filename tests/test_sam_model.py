"""tests/sam_model.py without a device: the numpy-fp32 restatement of cara_sam_perturb stays within the bound derived in that
module's docstring of the fp64 value -- on random inputs and on the hand-picked ones --, a contracted (fma) kernel is told apart
from the specified one, and the signed-zero and guard behaviour is the documented one."""
import numpy as np
import pytest

from tests import sam_model as M

F = np.float32


def _hold(p, g, rho, norm):
    got = M.perturb_f32(p, g, rho, norm)[0].astype(np.float64)
    err, b = np.abs(got - M.exact64(p, g, rho, norm)), M.bound(p, g, rho, norm)
    assert np.all(err <= b), (rho, norm, float(np.max(err / np.maximum(b, 1e-300))))
    return float(np.max(err / np.maximum(b, 1e-300)))


@pytest.mark.parametrize("rho", [0.05, 0.5, 2.0, 1e-3])
def test_restatement_within_the_derived_bound_on_random_inputs(rho):
    worst = 0.0
    for seed, (sp, sg) in enumerate(((1.0, 1.0), (0.02, 1e-3), (1e-3, 30.0), (1e6, 1e-6), (1e-20, 1e-20))):
        for n in (1, 5, 4099):
            p, g = M.random_pairs(n, 10 * seed + n, sp, sg)
            worst = max(worst, _hold(p, g, rho, M.l2_norm_f32([g])))
            worst = max(worst, _hold(p, g, rho, F(7.25)))              # (the kernel takes any norm it is handed)
    print(f"rho {rho}: worst |restatement - fp64| / bound {worst:.3f}")
    assert 0.05 < worst <= 1.0                                          # the bound is not slack by orders of magnitude either


def test_hand_picked_inputs():
    p, _ = M.random_pairs(64, 3)
    zero = np.zeros(64, np.float32)
    # norm = 0 with g = 0: scale = rho / 1e-12 is finite, s = 0, p comes back (no -0 among these weights)
    out, st = M.perturb_f32(p, zero, 0.05, F(0.0))
    assert np.array_equal(M.bits(out), M.bits(p)) and st[2] == F(0.05) / M.C12 and np.isfinite(st[2])
    _hold(p, zero, 0.05, F(0.0))
    # a tiny norm, where the 1e-12 matters: without it the scale would be 2.5 times as large
    g = (M.random_pairs(64, 4)[1] * F(1e-13)).astype(np.float32)
    norm = M.l2_norm_f32([g])
    assert 1e-13 < norm < 1e-11
    assert abs(float(M.scale_f32(0.05, norm)) / (0.05 / (float(norm) + 1e-12)) - 1.0) < 4 * M.U
    assert float(M.scale_f32(0.05, norm)) < 0.95 * 0.05 / float(norm)
    _hold(p, g, 0.05, norm)
    # the step has length rho (norm >> 1e-12): |e| = rho |g| / (|g| + 1e-12)
    p2, g2 = M.random_pairs(4099, 5, 0.02, 1e-3)
    e = M.perturb_f32(p2, g2, 0.05, M.l2_norm_f32([g2]))[0].astype(np.float64) - p2
    assert abs(np.sqrt(np.sum(e ** 2)) / 0.05 - 1.0) < 1e-4
    # a subnormal g: an exact input; with its own norm (subnormal too) the scale brings the product back into the normal range
    ps, gs = M.subnormal_grads(257, 6)
    assert np.all(np.abs(gs) < M.TINY) and np.all(gs != 0)
    _hold(ps, gs, 0.05, M.l2_norm_f32([gs]))
    _hold(ps, gs, 0.05, F(1.0))                                        # ... and with a norm that leaves the product subnormal
    _hold((ps * F(1e-38)).astype(np.float32), gs, 0.05, F(1.0))       # (subnormal weights too: the sum is exact)
    # a scale that underflows itself
    _hold(p, M.random_pairs(64, 8, 1.0, 1e30)[1], 1e-30, F(1e30))
    # rho = 0 gives p back for finite g, bit for bit
    pr, gr = M.random_pairs(4099, 7, 0.02, 1e3)
    out, st = M.perturb_f32(pr, gr, 0.0, M.l2_norm_f32([gr]))
    assert np.array_equal(M.bits(out), M.bits(pr)) and st[2] == 0.0
    assert np.isnan(M.perturb_f32([F(1.0)], [F(np.inf)], 0.0, F(1.0))[0][0])      # ... and not for an infinite one


def test_a_contracted_kernel_is_told_apart():
    # the stated input: p = 1, g = 1 + 2^-22, rho = 1, norm = 3 -- scale = fl(1 / fl(3 + 1e-12)) = 0.33333334
    p, g = [F(1.0)], [F(1.0 + 2.0 ** -22)]
    a, b = M.perturb_f32(p, g, 1.0, F(3.0))[0], M.perturb_fma(p, g, 1.0, F(3.0))
    assert M.scale_f32(1.0, 3.0) == F(0.33333334)
    assert M.bits(a)[0] != M.bits(b)[0] and abs(int(M.bits(a)[0]) - int(M.bits(b)[0])) == 1
    # both are inside the bound (the fma value is the more accurate one): only a bitwise comparison separates them
    for v in (a, b):
        assert np.all(np.abs(v.astype(np.float64) - M.exact64(p, g, 1.0, F(3.0))) <= M.bound(p, g, 1.0, F(3.0)))
    # ... and on inputs like a step's (weights ~ 0.02, gradients ~ 1e-3) a few per cent of the elements differ
    p, g = M.random_pairs(8193, 11, 0.02, 1e-3)
    norm = M.l2_norm_f32([g])
    differ = int(np.count_nonzero(M.bits(M.perturb_f32(p, g, 0.05, norm)[0]) != M.bits(M.perturb_fma(p, g, 0.05, norm))))
    print(f"fma vs two roundings: {differ} of 8193 elements differ")
    assert differ > 80


def test_signed_zeros_and_guards_are_the_documented_ones():
    nz, pz = F(-0.0), F(0.0)
    one = lambda p, g, rho=0.05, norm=1.0: int(M.bits(M.perturb_f32([p], [g], rho, F(norm))[0])[0])   # noqa: E731
    NZ, PZ = int(M.bits([nz])[0]), 0
    assert one(nz, pz) == PZ and one(nz, nz) == NZ and one(pz, nz) == PZ and one(pz, pz) == PZ
    assert one(nz, F(2.0), rho=0.0) == PZ and one(nz, F(-2.0), rho=0.0) == NZ       # rho = 0: s = +-0 with g's sign
    assert one(nz, pz, norm=0.0) == PZ and one(F(1.5), pz, norm=0.0) == int(M.bits([F(1.5)])[0])
    # guards: p untouched (its bits, a NaN payload included), the scale reported 0, the carry reported as read
    p = np.array([1.0, -0.0, 2.0 ** -140, 0.0], np.float32)
    p[3:4].view(np.int32)[0] = 0x7fc12345
    g = np.ones(4, np.float32)
    for norm, found in ((1.0, 1.0), (1.0, 3.0), (1.0, np.nan), (np.nan, None), (np.inf, 0.0), (-np.inf, None)):
        out, st = M.perturb_f32(p, g, 0.05, F(norm), found)
        assert np.array_equal(M.bits(out), M.bits(p)) and st[2] == 0.0 and st[3] == 0.0, (norm, found)
        assert M.bits(st[:2]).tolist() == M.bits([F(0.0 if found is None else found), F(norm)]).tolist()
    out, st = M.perturb_f32(p[:3], g[:3], 0.05, F(1.0), 0.0)
    assert st[0] == 0.0 and st[2] == M.scale_f32(0.05, 1.0) and not np.array_equal(M.bits(out), M.bits(p[:3]))
