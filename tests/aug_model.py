"""Restatements and DERIVED bounds of the jittered resident feed (cara_im2col_patches_u8_rows_aug), shared by
tests/test_aug_model.py (host) and tests/test_aug_gpu.py (device).  numpy fp32 in the kernels' order; nothing here is fitted to a
device.

What is restated to the bit: the unmixed bilinear value `u` (crop_axis / crop_value are compiled with the default contraction, and
their gfx950 instruction stream fuses the position's multiply-subtract and every a + f (b - a): `fma32` below is an exact fused
multiply-add), the colour chain (plain operators under `fp contract(off)`: one rounding per product and per sum), and the fixed tree
of aug_gray_mean_kernel.

The bounds (u = 2^-24, gamma(k) = k u / (1 - k u)), against the same formula in float64 on the same fp32 inputs:
  slot:   v' = clamp(fl(fl(f v) + fl(fl(1 - f) d)))  -- three roundings plus that of 1 - f:
          |v' - (f v + (1 - f) d)| <= u (|f v| + 2 |1 - f| |d| + |f v + (1 - f) d|) (1 + 2^-20)  +  f dv + |1 - f| dd
          (dv, dd: what v and d carry in; the clamp is 1-Lipschitz and 0, 255 are exact).
  gray:   (wr r + wg g) + wb b, all terms >= 0, longest path product, sum, sum:   gamma(3) gray + (wr dr + wg dg + wb db).
  mean:   thread: ceil(n / 4096) sequential additions; butterfly 6; waves 3; workgroups 15; one division.  With gray's 3 the
          longest path is m = ceil(n / 4096) + 28, all terms >= 0:   |M - M64| <= gamma(m) M64 + max(d gray).
"""
import numpy as np
import torch

U = 2.0 ** -24
F = np.float32
GROUPS = 16                                   # AUG_GROUPS of feed.hip: workgroups per sample, part of the tree
WR, WG, WB = F(0.2989), F(0.587), F(0.114)


def gamma(k):
    return k * U / (1.0 - k * U)


def bits(x):
    return int(torch.tensor(x, dtype=torch.float32).view(torch.int32))


def row(ops=(), erase=(0, 0, 0, 0), emode=0, eseed=0, pad=(0, 0, 0, 0)):
    """one table row from [(op, f), ...] (up to three), an erase rectangle (ex0, ey0, ew, eh), emode, eseed"""
    slots = list(ops) + [(0, 0.0)] * (3 - len(ops))
    words = []
    for op, f in slots:
        words += [int(op), bits(f) if op else 0]
    seed = int(eseed) & 0xffffffff
    return words + [int(v) for v in erase] + [int(emode), seed - (1 << 32) if seed >= 1 << 31 else seed] + [int(v) for v in pad]


def table(rows):
    return torch.tensor(rows, dtype=torch.int32)


def row_slots(r):
    """[(op, fp32 factor)] x 3 of a table row (a list or tensor of 16 ints)"""
    r = [int(v) for v in (r.tolist() if torch.is_tensor(r) else r)]
    return [(r[2 * k], np.array([r[2 * k + 1]], dtype=np.int32).view(np.float32)[0]) for k in range(3)]


def contrast_at(r):
    return next((k for k, (op, _) in enumerate(row_slots(r)) if op == 2), 3)


# ---- the unmixed value, to the bit -------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fl32(a b + c) with ONE rounding, for fp32 arrays: the product is exact in float64; the sum is rounded to odd there (TwoSum's
    exact remainder decides), and 53 >= 24 + 2 bits make the final rounding to fp32 the correct one"""
    a, b, c = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    s, err = np.broadcast_arrays(s, err)
    even = (s.copy().view(np.int64) & 1) == 0
    nxt = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & even, nxt, s).astype(np.float32)


def _axis(n_out, n_box, flip):
    o = np.arange(n_out)
    of = (n_out - 1 - o if flip else o).astype(np.float32)
    ratio = F(n_box) / F(n_out)
    s = np.maximum(fma32(of + F(0.5), ratio, F(-0.5)), F(0))
    i0 = np.minimum(s.astype(np.int64), n_box - 1)
    return i0, np.minimum(i0 + 1, n_box - 1), (s - i0.astype(np.float32)).astype(np.float32)


def crop_f32(pixels_u8, rows, boxes, Hi, Wi):
    """crop_value of every output pixel: fp32 [B,C,Hi,Wi], bit for bit what the kernels hold before the chain"""
    px = pixels_u8.cpu().numpy()
    out = np.empty((len(rows), px.shape[1], Hi, Wi), dtype=np.float32)
    for b, (r, (x0, y0, w, h, flip)) in enumerate(zip(rows, boxes)):
        src = px[r, :, y0:y0 + h, x0:x0 + w].astype(np.float32)
        iy0, iy1, fy = _axis(Hi, h, False)
        ix0, ix1, fx = _axis(Wi, w, flip != 0)
        top0, top1 = src[:, iy0][:, :, ix0], src[:, iy0][:, :, ix1]
        bot0, bot1 = src[:, iy1][:, :, ix0], src[:, iy1][:, :, ix1]
        t = fma32(fx[None, None, :], top1 - top0, top0)
        u = fma32(fx[None, None, :], bot1 - bot0, bot0)
        out[b] = fma32(fy[None, :, None], u - t, t)
    return out


# ---- the chain and the tree, to the bit --------------------------------------------------------------------------------------
def gray_f32(x):
    return ((WR * x[0] + WG * x[1]) + WB * x[2]).astype(np.float32)


def tree_mean(gray):
    """aug_gray_mean_kernel + aug_gray_mean_reduce_kernel on the gray values of one image (fp32, any shape, row-major pixels)"""
    g = np.asarray(gray, dtype=np.float32).reshape(-1)
    n = g.size
    partial = np.zeros(GROUPS, dtype=np.float32)
    lanes = np.arange(64)
    for k in range(GROUPS):
        acc = np.zeros(256, dtype=np.float32)
        q = k * 256 + np.arange(256)
        while (q < n).any():
            live = q < n
            acc[live] = acc[live] + g[q[live]]
            q = q + 256 * GROUPS
        acc = acc.reshape(4, 64)
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lanes ^ off]
        w = acc[:, 0]
        partial[k] = ((w[0] + w[1]) + w[2]) + w[3]
    t = partial[0]
    for k in range(1, GROUPS):
        t = F(t + partial[k])
    return F(t / F(n))


def mean_path(n):
    """additions and the division on the longest path from a pixel's channel values to M (gray's three included)"""
    return -(-n // (256 * GROUPS)) + 6 + 3 + (GROUPS - 1) + 1 + 3


def slot_f32(v, d, f, slip=None):
    f = F(f)
    omf = F(F(1) - f)
    if slip == "fused":
        s = fma32(f, v, (omf * d).astype(np.float32))
    else:
        s = ((f * v).astype(np.float32) + (omf * d).astype(np.float32)).astype(np.float32)
    return s if slip == "no clamp" else np.minimum(np.maximum(s, F(0)), F(255))


def chain_f32(x, r, upto=3, M=None, slip=None):
    """slots [0, upto) of row r on one image x fp32 [3,Hi,Wi] in the kernel's order -> (image, M used or None)"""
    x = np.asarray(x, dtype=np.float32).copy()
    used = None
    for k, (op, f) in enumerate(row_slots(r)):
        if k >= upto or op == 0:
            continue
        if op == 3:
            d = gray_f32(x) if slip != "bf16 weights" else _gray_slipped(x)
        elif op == 2:
            used = d = tree_mean(gray_f32(x)) if M is None else F(M)
        else:
            d = F(0)
        x = np.stack([slot_f32(x[c], d, f, slip) for c in range(3)])
    return x, used


def _gray_slipped(x):
    w = [F(torch.tensor(float(v)).to(torch.bfloat16).float().item()) for v in (WR, WG, WB)]
    return ((w[0] * x[0] + w[1] * x[1]) + w[2] * x[2]).astype(np.float32)


def stat_f32(u_b, r):
    """stat[b] of the device: the tree's mean of gray after the slots that precede the contrast slot (None without one)"""
    at = contrast_at(r)
    if at == 3:
        return None
    x, _ = chain_f32(u_b, r, upto=at)
    return tree_mean(gray_f32(x))


def sequential_mean(gray):
    """a slipped mean: one running fp32 sum over the pixels"""
    t = F(0)
    for v in np.asarray(gray, dtype=np.float32).reshape(-1):
        t = F(t + v)
    return F(t / F(np.asarray(gray).size))


# ---- the same chain in float64, with the derived bound carried along -----------------------------------------------------------
def chain_bound(x, r, e0=0.0):
    """(v, e, M, eM): the chain of row r in float64 on the image x [3,Hi,Wi] (fp32, or float64 with every element known to within
    e0) and the derived bound e >= |chain_f32 - v| per element; M, eM: the contrast statistic and its bound (None without a
    contrast slot)"""
    v = np.asarray(x).astype(np.float64)
    e = np.full_like(v, float(e0))
    w = np.array([WR, WG, WB], dtype=np.float64).reshape(3, 1, 1)
    slack = 1.0 + 2.0 ** -20
    M = eM = None
    n = v[0].size
    for op, f in row_slots(r):
        if op == 0:
            continue
        f = float(f)
        gray = (w * v).sum(0)
        e_gray = gamma(3) * gray + (w * e).sum(0)
        if op == 3:
            d, ed = gray, e_gray
        elif op == 2:
            M = d = gray.mean()
            eM = ed = gamma(mean_path(n)) * M + e_gray.max()
        else:
            d, ed = 0.0, 0.0
        exact = f * v + (1.0 - f) * d
        e = U * (np.abs(f * v) + 2 * abs(1.0 - f) * np.abs(d) + np.abs(exact)) * slack + f * e + abs(1.0 - f) * ed
        v = np.clip(exact, 0.0, 255.0)
    return v, e, M, eM


# ---- through the normalisation -----------------------------------------------------------------------------------------------
IMAGENET_STD_MIN = 0.224
# tests/mix_model.py: an unmixed element of these shapes is within E_CROP of float64 after normalisation, a blend adds 3 u / std
E_CROP = 1.3e-4
E_CROP_BYTES = 7.1e-3        # the same before normalisation, in byte steps (tests/test_augmented_feed_gpu.py's derivation)
E_BLEND = 3 * U / IMAGENET_STD_MIN


def normalized_bound(e_byte_scale, std):
    """a 0..255-scale error e through (v / 255 - mean) / std: e / (255 std), plus the three roundings of the normalisation of a
    value |x| < 2.7 (5e-7, as in tests/mix_model.py)"""
    return e_byte_scale / (255.0 * std) + 5e-7
