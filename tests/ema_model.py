"""Host-side model of cara_ema_update (cara_amd/csrc/optim.hip, include/cara_hip.h): a numpy-fp32 restatement of the two-branch
update, an fp64 value of the same formula, and the error bound DERIVED from the operation count.  tests/test_ema_model.py proves
the bound on the restatement without a device; tests/test_ema_gpu.py holds the device to the restatement bit for bit.

The update, per element, every operation one IEEE fp32 operation (w = 1 - decay, an fp32 number in [0, 1]):
    d = p - e
    w <  0.5:   e' = e + w * d                    (branch 1)
    otherwise:  e' = p - d * (1 - w)              (branch 2; 1 - w is exact for w in [0.5, 1]: Sterbenz)
Each of the three operations rounds once, relative error at most u = 2^-24 where no underflow occurs:
    branch 1:  e' = (e + w d (1 + d1)(1 + d2))(1 + d3)   ->  |e' - exact| <= u |e| + 3 u w |d| + O(u^2)
    branch 2:  e' = (p - (1 - w) d (1 + d1)(1 + d2))(1 + d3)   ->  |e' - exact| <= u |p| + 3 u (1 - w) |d| + O(u^2)
The O(u^2) terms (at most ~3 u^2 of the second summand) and the fp64 evaluation of `exact` (2^-53 relative per operation) are far
inside the slack factor 1 + 2^-20.
Gradual underflow: additions and subtractions are exact when their result is subnormal, but a PRODUCT below 2^-126 is rounded to
a multiple of 2^-149, an absolute error of up to 2^-150 that no relative bound covers (e = 0, p = 2^-149, w = 0.25 gives 0 where
the formula gives 2^-151).  The bound above therefore holds on subnormal inputs whose products are exact or round with a relative
error of u -- `subnormal_pairs` below: e, p and d multiples of 2^-135 -- and UNDERFLOW_ABS states what holds where they are not.
Signed zeros: p == e gives e back bitwise except e = p = -0 at w < 0.5, which gives +0 (d = +0, -0 + +0 = +0).
"""
import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
UNDERFLOW_ABS = 2.0 ** -150          # half the smallest subnormal: the most a product below 2^-126 is off by
BELOW_HALF = np.nextafter(np.float32(0.5), np.float32(0.0))
WEIGHTS = tuple(np.float32(w) for w in (0.0, 2.0 ** -13, 0.25, BELOW_HALF, 0.5, 0.75, 1.0))
EXTRA_WEIGHTS = (np.float32(0.1), np.float32(0.9), np.float32(1.0 - 0.9998))   # factors that are no power of two, both branches
MAX_TENSORS = 32                    # CARA_ADAMW_MAX_TENSORS


def update_f32(e, p, w):
    """the kernel's arithmetic in numpy fp32, one rounding per operation -> the new e (inputs are left unchanged)"""
    e, p, w = np.asarray(e, np.float32), np.asarray(p, np.float32), np.float32(w)
    d = p - e
    if w < np.float32(0.5):
        s = w * d
        return (e + s).astype(np.float32)
    s = d * (np.float32(1.0) - w)
    return (p - s).astype(np.float32)


def update_fma(e, p, w):
    """what a contracted kernel computes: the product and the last sum fused, ONE rounding for both (the product of two fp32
    numbers is exact in fp64; the fp64 sum is then rounded to fp32)"""
    e, p, w = np.asarray(e, np.float32), np.asarray(p, np.float32), np.float32(w)
    d = (p - e).astype(np.float64)
    if w < np.float32(0.5):
        return (e.astype(np.float64) + np.float64(w) * d).astype(np.float32)
    return (p.astype(np.float64) - d * np.float64(np.float32(1.0) - w)).astype(np.float32)


def exact64(e, p, w):
    """the same formula in fp64 from the fp32-rounded w"""
    e, p, w = np.asarray(e, np.float32).astype(np.float64), np.asarray(p, np.float32).astype(np.float64), np.float64(np.float32(w))
    if w < 0.5:
        return e + w * (p - e)
    return p - (p - e) * (1.0 - w)


def bound(e, p, w):
    """the derived bound on |update_f32 - exact64|, per element"""
    e, p, w = np.asarray(e, np.float32).astype(np.float64), np.asarray(p, np.float32).astype(np.float64), np.float64(np.float32(w))
    if w < 0.5:
        return SLACK * U * (np.abs(e) + 3.0 * w * np.abs(p - e))
    return SLACK * U * (np.abs(p) + 3.0 * (1.0 - w) * np.abs(p - e))


def decay_at(decay, warmup, t):
    """the schedule of cara_amd/ema.py, restated: t = updates already made"""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def weight_at(decay, warmup, t):
    return np.float32(1.0 - decay_at(decay, warmup, t))


# ---- inputs (seeded; every function returns fresh arrays) -------------------------------------------------------------------------
def random_pairs(n, seed, scale=1.0):
    r = np.random.default_rng(seed)
    return (r.standard_normal(n) * scale).astype(np.float32), (r.standard_normal(n) * scale).astype(np.float32)


def near_pairs(n, seed):
    """p within an ulp of e (one step down, equal, one step up), and the signed zeros"""
    e = random_pairs(n, seed)[0]
    step = np.random.default_rng(seed + 1).integers(-1, 2, n)
    p = np.where(step < 0, np.nextafter(e, np.float32(-np.inf)), np.where(step > 0, np.nextafter(e, np.float32(np.inf)), e))
    return e, p.astype(np.float32)


def lopsided_pairs(n, seed, big_e=True):
    """|e| >> |p| (or the reverse): 1e30 against 1e-30, and 1e6 against 1"""
    a, b = random_pairs(n, seed)
    big = np.where(np.arange(n) % 2 == 0, np.float32(1e30), np.float32(1e6))
    small = np.where(np.arange(n) % 2 == 0, np.float32(1e-30), np.float32(1.0))
    return ((a * big).astype(np.float32), (b * small).astype(np.float32)) if big_e else ((a * small).astype(np.float32), (b * big).astype(np.float32))


def subnormal_pairs(n, seed):
    """e and p subnormal, multiples of 2^-135 = 2^14 x 2^-149 with |.| < 2^-126: d is exact, and every product with a weight of
    WEIGHTS is exact or rounds with a relative error below u (see the module docstring)"""
    r = np.random.default_rng(seed)
    j = r.integers(-511, 512, (2, n))
    j[j == 0] = 1
    return np.ldexp(j[0].astype(np.float64), -135).astype(np.float32), np.ldexp(j[1].astype(np.float64), -135).astype(np.float32)


def kernel_case(seed=5):
    """the 32-tensor call of the GPU test: sizes 1, 3, 4, 5, 1023, 1024, 1025, 4099 four times over -> [(e, p)] in fp32, with a few
    elements of every tensor at the fixed point p == e and one a signed zero"""
    sizes = (1, 3, 4, 5, 1023, 1024, 1025, 4099) * 4
    out = []
    for i, n in enumerate(sizes):
        e, p = random_pairs(n, seed * 100 + i)
        p[::7] = e[::7]
        if n > 4:
            e[4], p[4] = np.float32(-0.0), np.float32(0.0)
        out.append((e, p))
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)
