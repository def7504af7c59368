"""Restatements and the DERIVED bound of the global-norm clip (cara_grad_clip, cara_amd/csrc/optim.hip), shared by
tests/test_grad_clip_model.py (host) and tests/test_grad_clip_gpu.py / tests/test_accumulate_gpu.py (device).  In the manner of
tests/mix_model.py: a float64 definition, the kernel's own operations in its own order in numpy fp32, and a bound counted from the
roundings on the longest path of that order; nothing here is fitted to a device.

The tree (the comment above CLIP_CHUNK in optim.hip): a chunk is 8192 consecutive elements, 256 threads per workgroup.
  1. thread t: acc = 0; for j = 0 .. 7, c = 0 .. 3: acc += g[8192 chunk + 4 (256 j + t) + c]^2   -- 32 squares (one rounding each),
     32 sequential additions of which the first (to 0) is exact: 31;
  2. wave_sum's butterfly over the wave's 64 lanes (32, 16, 8, 4, 2, 1 apart): 6 additions;
  3. the four wave sums left to right: 3 additions                                                 -> partial[chunk]
  4. thread t: acc = 0; for q = t, t + 256, ...: acc += partial[q] -- at most ceil(chunks / 256) additions (counted in full) --
     then 2. and 3. again: 6 + 3                                                                   -> total
so m(n) = 31 + 6 + 3 + ceil(chunks / 256) + 6 + 3 additions lie on the longest path from a square to the total.

The bound.  All terms are >= 0, so the computed total is sum_i g_i^2 (1 + theta_i) with |theta_i| <= gamma(m + 1) (m additions and
the square's own rounding; gamma(k) = k u / (1 - k u), u = 2^-24: Higham, Accuracy and Stability, lemma 3.1), i.e. within
gamma(m + 1) of the exact total, relatively; sqrtf (correctly rounded) halves that and adds one rounding:
    |norm_dev - norm_64| / norm_64  <=  gamma(m + 1) / 2 + u (1 + ...)  <=  gamma(m + 2)  =: NORM_BOUND(n).
(gamma over the additions on the longest path, plus one rounding per square and per sqrtf.)  It needs the
squares to be normal fp32 numbers or exactly 0 (2^-63 <= |g| <= 2^63): the tests' magnitudes are 1e-6 .. 1e3.
coef = min(1, max_norm / (norm + 1e-6f)): the addition and the division round once each, the clamp is monotone; an element is one
more product.  With coef_64 <= 1:
    |g_dev - g_64 coef_64|  <=  |g| (NORM_BOUND(n) + 3 u)
-- the cross terms (<= 3 u NORM_BOUND) are inside gamma's denominator: gamma(k) >= k u + k^2 u^2 and k = m + 2 >= 52.
"""
import math

import numpy as np

from oracle.small_kernels import U, gamma

CHUNK = 8192          # CLIP_CHUNK of optim.hip
THREADS = 256
EPS = float(np.float32(1e-6))     # torch's 1e-6, as the fp32 constant the kernel adds
FLAT_R16_C100 = 121925            # the flat gradient buffer at rank 16 / 100 classes, with its found-inf word
SIZES = (1, CHUNK - 1, CHUNK, CHUNK + 1, FLAT_R16_C100)


def chunks(n):
    return -(-n // CHUNK)


def additions(n):
    """additions on the longest path of the tree above"""
    return 31 + 6 + 3 + -(-chunks(n) // THREADS) + 6 + 3


def norm_bound(n):
    """bound on |norm_dev - norm_64| / norm_64 (and on the same of out[0])"""
    return gamma(additions(n) + 2)


def elem_bound(n):
    """per element: |g_dev - g_64 coef_64| <= |g| elem_bound(n); also the bound on |coef_dev - coef_64| / coef_64"""
    return norm_bound(n) + 3 * U


def buffer(n, seed):
    """seeded fp32 test buffer: signs at random, magnitudes log-uniform over 1e-6 .. 1e3"""
    r = np.random.default_rng(seed)
    mag = 10.0 ** r.uniform(-6.0, 3.0, n)
    return (mag * r.choice([-1.0, 1.0], n)).astype(np.float32)


def clip64(g, max_norm):
    """torch.nn.utils.clip_grad_norm_(norm_type=2) in float64 -> (norm, coef, clipped g)"""
    g64 = np.asarray(g, dtype=np.float64)
    norm = math.sqrt(math.fsum((g64 * g64).tolist()))
    coef = min(1.0, float(max_norm) / (norm + EPS))
    return norm, coef, g64 * coef


def _block_sum(acc):
    """steps 2 and 3: fp32 [P, 256] -> [P]"""
    acc = acc.reshape(-1, 4, 64)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lanes ^ off]
    w = acc[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def partials_f32(g):
    """launch 1 in numpy fp32: one sum of squares per chunk, in the kernel's order"""
    g = np.asarray(g, dtype=np.float32)
    P = chunks(g.size)
    pad = np.zeros(P * CHUNK, dtype=np.float32)
    pad[:g.size] = g
    x = pad.reshape(P, 8, THREADS, 4)            # [chunk][j][t][c]: element 8192 chunk + 4 (256 j + t) + c
    sq = x * x
    acc = np.zeros((P, THREADS), dtype=np.float32)
    for j in range(8):
        for c in range(4):
            acc = acc + sq[:, j, :, c]
    out = _block_sum(acc)
    assert out.dtype == np.float32
    return out


def total_f32(partials):
    """step 4: what every workgroup of launch 2 computes"""
    P = partials.size
    R = -(-P // THREADS)
    pad = np.zeros(R * THREADS, dtype=np.float32)
    pad[:P] = partials
    pad = pad.reshape(R, THREADS)
    acc = np.zeros(THREADS, dtype=np.float32)
    for r in range(R):
        acc = acc + pad[r]
    return _block_sum(acc[None])[0]


def clip_f32(g, max_norm):
    """the two launches in numpy fp32 -> (norm, coef, g afterwards): the kernel's operations in its order"""
    g = np.asarray(g, dtype=np.float32)
    norm = np.sqrt(total_f32(partials_f32(g)))
    c = np.float32(max_norm) / (norm + np.float32(1e-6))
    coef = c if (c < 1 or c != c) else np.float32(1.0)
    assert norm.dtype == np.float32 and np.float32(coef).dtype == np.float32
    return norm, np.float32(coef), (g if coef == 1 else g * np.float32(coef))
