"""Host-side model of cara_sam_perturb / cara_sam_restore (cara_amd/csrc/optim.hip, include/cara_hip.h): a numpy-fp32 restatement
of the scale and the update, an fp64 value of the same formula, and the error bound DERIVED from the operation count.
tests/test_sam_model.py proves the bound on the restatement without a device; tests/test_sam_gpu.py holds the device to the
restatement bit for bit.

The move, every operation one IEEE fp32 operation (rho >= 0 and norm fp32 numbers, c = float32(1e-12), the constant of the published
SAM implementation -- a definition, not a tolerance):
    den   = norm + c                      rounding 1
    scale = rho / den                     rounding 2        (both the same in every thread)
    s     = scale * g                     rounding 3
    p'    = p + s                         rounding 4
Each rounds once, relative error at most u = 2^-24 where no underflow occurs.  With S = rho / (norm + c) the exact quotient:
    scale = S (1 + d2) / (1 + d1),   s = S g (1 + d2)(1 + d3) / (1 + d1),   p' = (p + s)(1 + d4)
    |p' - (p + S g)| <= u |p + S g| + (1 + u) |S g| (3 u + O(u^2)) <= u |p| + 4 u |S g| + O(u^2)
The O(u^2) terms (below 7 u^2 |S g|) and the fp64 evaluation of the exact value (2^-53 relative per operation, four operations) are far
inside the slack factor 1 + 2^-20.
Gradual underflow: an addition is exact when its result is subnormal, but a PRODUCT or QUOTIENT below 2^-126 is rounded to a multiple
of 2^-149, an absolute error of up to 2^-150 that no relative bound covers.  The bound therefore adds UNDERFLOW_ABS where |S g| is
below 2^-126 (rounding 3) and |g| UNDERFLOW_ABS (1 + 3 u) where S itself is (rounding 2, carried through the product).  A subnormal g
is an exact input: its product with a scale that brings it back into the normal range rounds like any other.
Guards (no arithmetic, so no bound): a non-zero (or NaN) found-inf word, or a norm that is not finite, leaves p as it is; the scale
reported is then 0.  The backup is p's bits in every case, and the restore copies them back: -0, subnormals and NaN payloads return.
Signed zeros of the move: p' = p bitwise wherever s is a zero, EXCEPT p = -0 with s = +0, which gives +0 (IEEE: -0 + +0 = +0).
s = scale * g carries g's sign (scale >= 0), so g = +0, and any g >= 0 under rho = 0, turn a -0 weight into +0 for the second pass;
g = -0 keeps it.  The restore brings -0 back either way.  rho = 0 gives p back only for finite g: 0 * inf is NaN.
"""
import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
UNDERFLOW_ABS = 2.0 ** -150          # half the smallest subnormal: the most a product or quotient below 2^-126 is off by
TINY = 2.0 ** -126                   # the smallest normal fp32 number
C12 = np.float32(1e-12)
MAX_TENSORS = 32                     # CARA_ADAMW_MAX_TENSORS
LENGTHS = (1, 3, 4, 5, 255, 256, 257, 8191, 8192, 8193, 768 * 100 + 100)   # chunk (1024) and float4 edges, the head's weight + bias


def scale_f32(rho, norm):
    """the kernel's scale: two roundings"""
    with np.errstate(all="ignore"):
        den = np.float32(norm) + C12
        return np.float32(np.float32(rho) / den)


def moves(norm, found_inf=None):
    """whether the kernel moves p at all: no carry (a NaN word counts as one) and a finite norm"""
    carried = found_inf is not None and not (np.float32(found_inf) == np.float32(0.0))
    return (not carried) and bool(np.isfinite(np.float32(norm)))


def perturb_f32(p, g, rho, norm, found_inf=None):
    """the kernel's arithmetic in numpy fp32, one rounding per operation -> (the new p, state[4]); inputs are left unchanged"""
    p, g = np.asarray(p, np.float32), np.asarray(g, np.float32)
    carry = np.float32(0.0) if found_inf is None else np.float32(found_inf)
    if not moves(norm, found_inf):
        return p.copy(), np.array([carry, np.float32(norm), 0.0, 0.0], np.float32)
    scale = scale_f32(rho, norm)
    with np.errstate(all="ignore"):
        s = (scale * g).astype(np.float32)
        out = (p + s).astype(np.float32)
    return out, np.array([carry, np.float32(norm), scale, 0.0], np.float32)


def perturb_fma(p, g, rho, norm):
    """what a contracted kernel computes: the product and the sum fused, ONE rounding for both (the product of two fp32 numbers is
    exact in fp64; the fp64 sum is then rounded to fp32)"""
    p, g = np.asarray(p, np.float32), np.asarray(g, np.float32)
    scale = np.float64(scale_f32(rho, norm))
    with np.errstate(all="ignore"):
        return (p.astype(np.float64) + scale * g.astype(np.float64)).astype(np.float32)


def exact64(p, g, rho, norm):
    """the same formula in fp64 from the fp32 inputs (and the fp32-rounded 1e-12)"""
    p, g = np.asarray(p, np.float32).astype(np.float64), np.asarray(g, np.float32).astype(np.float64)
    S = np.float64(np.float32(rho)) / (np.float64(np.float32(norm)) + np.float64(C12))
    return p + S * g


def bound(p, g, rho, norm):
    """the derived bound on |perturb_f32 - exact64|, per element (finite inputs, a norm >= 0)"""
    p, g = np.asarray(p, np.float32).astype(np.float64), np.asarray(g, np.float32).astype(np.float64)
    S = np.float64(np.float32(rho)) / (np.float64(np.float32(norm)) + np.float64(C12))
    sg = np.abs(S * g)
    b = SLACK * U * (np.abs(p) + 4.0 * sg)
    b = b + np.where(sg < TINY, UNDERFLOW_ABS, 0.0)
    if S < TINY:
        b = b + np.abs(g) * UNDERFLOW_ABS * (1.0 + 3.0 * U)
    return b


def l2_norm_f32(gs):
    """a global L2 norm of the tensors gs as an fp32 number (fp64 sum, rounded once): an INPUT of the cases below -- the kernel takes
    any norm it is handed; the device's own comes from cara_grad_clip (tests/optim_model.py)"""
    return np.float32(np.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in gs)))


# ---- inputs (seeded; every function returns fresh arrays) -------------------------------------------------------------------------
def random_pairs(n, seed, scale_p=1.0, scale_g=1.0):
    r = np.random.default_rng(seed)
    return (r.standard_normal(n) * scale_p).astype(np.float32), (r.standard_normal(n) * scale_g).astype(np.float32)


def subnormal_grads(n, seed):
    """g subnormal (multiples of 2^-149 below 2^-126), p ordinary"""
    r = np.random.default_rng(seed)
    j = r.integers(-(1 << 22), 1 << 22, n)
    j[j == 0] = 1
    return random_pairs(n, seed + 1)[0], np.ldexp(j.astype(np.float64), -149).astype(np.float32)


def kernel_case(ntensors, seed=7, nan=False):
    """the tensors of one GPU call: lengths LENGTHS in turn -> [(p, g)] in fp32.  Every tensor longer than 8 holds the special
    values a copy must keep and a move must treat as stated above: -0 weights against +0, -0 and a positive gradient, a subnormal
    weight, a subnormal gradient, a zero gradient and, with ``nan`` (the cases in which nothing is computed on it: which NaN an
    addition returns is the hardware's choice), a NaN weight with a payload"""
    out = []
    for i in range(ntensors):
        n = LENGTHS[i % len(LENGTHS)]
        p, g = random_pairs(n, seed * 1000 + i, scale_p=0.02, scale_g=1e-3)
        if n > 8:
            p[0], g[0] = np.float32(-0.0), np.float32(0.0)
            p[1], g[1] = np.float32(-0.0), np.float32(-0.0)
            p[2], g[2] = np.float32(-0.0), np.float32(1e-3)
            p[3] = np.float32(2.0 ** -140)
            g[4] = np.float32(2.0 ** -140)
            g[5] = np.float32(0.0)
            if nan:
                p[6:7].view(np.int32)[0] = 0x7fc12345
        out.append((p, g))
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)
