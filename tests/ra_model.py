"""Restatement, to the bit, of the RandAugment feed (cara_im2col_patches_u8_rows_ra), shared by tests/test_ra_model.py (host) and
tests/test_ra_gpu.py (device).  numpy fp32 in the kernels' order; nothing here is fitted to a device.

The geometry of a non-identity matrix is compiled under `fp contract(off)`: every numpy fp32 product and sum below is the kernel's
one IEEE operation.  The identity matrix takes crop_axis / crop_value, whose gfx950 code fuses: tests/aug_model.crop_f32 (with its
exact fma32) is that path.  Quantisation is rint (half to even); the lookup slots and the statistic tables are integer arithmetic,
written here as plain Python loops (cara_amd.data.ra_lut is the vectorised form the two are compared with).  The jitter chain, its
tree mean and the Mixup blend (one fused multiply-add) are tests/aug_model's.

The bound of the geometry against the same formula in float64 on the same fp32 matrix (u = 2^-24), used by test_ra_model.py:
  position:  p = fl(fl(fl(m0 x) + fl(m1 y)) + m2), x and y exact:  |p - p64| <= 3 u A (1 + 2^-20),  A = |m0| x + |m1| y + |m2|
  axis:      s = max(fl(fl(pf fl(w / Wi)) - 0.5), 0), pf = p or fl(Wi - p) (one more rounding of at most u Wi):
             |s - s64| <= (w / Wi) (dp + u Wi) + 3 u (Wi (w / Wi) + 0.5) (1 + 2^-20)                                  =: ds
  value:     bilinear in (sx, sy), continuous across the index steps, slope at most D = the largest difference of two adjacent
             source bytes per axis; its own five roundings are at most 5 u 255 (1 + 2^-20):
             |v - v64| <= D (dsx + dsy) + 5 u 255 (1 + 2^-20)
A pixel whose float64 u or v lies within dp of 0, Wi or Hi may fall on the other side of the inside test: such pixels are set aside
with those within 2^-10 of a half-integer.
"""
import numpy as np
import torch

from tests import aug_model as G
from tests.aug_model import F, crop_f32, fma32

U = 2.0 ** -24
ONE = 0x3f800000
POSTERIZE, SOLARIZE, SOLARIZE_ADD, INVERT, AUTOCONTRAST, EQUALIZE = 1, 2, 3, 4, 5, 6
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def fbits(x):
    return int(np.array([x], dtype=np.float32).view(np.int32)[0])


def row(slots=(), matrix=IDENTITY, fill=0, pad=(0, 0, 0)):
    """one ra row from [(op, arg), ...] (up to three), six matrix values (numbers, rounded to fp32, or ("bits", int) words), a fill"""
    slots = list(slots) + [(0, 0)] * (3 - len(slots))
    words = [int(v) for s in slots for v in s]
    words += [int(m[1]) if isinstance(m, tuple) else fbits(m) for m in matrix]
    return words + [int(fill)] + [int(v) for v in pad]


def table(rows):
    return torch.tensor(rows, dtype=torch.int32)


def is_identity(r):
    return [int(v) for v in r[6:12]] == [ONE, 0, 0, 0, ONE, 0]


def _words(r):
    return [int(v) for v in (r.tolist() if torch.is_tensor(r) else r)]


def geometry_f32(px_u8, r, box, rw, Hi, Wi):
    """the value before quantisation of every output pixel of one sample: fp32 [3,Hi,Wi]"""
    rw = _words(rw)
    if is_identity(rw):
        return crop_f32(px_u8, [r], [box], Hi, Wi)[0]
    x0, y0, w, h, flip = (int(v) for v in box)
    m = np.array(rw[6:12], dtype=np.int64).astype(np.uint32).view(np.float32)
    src = px_u8.cpu().numpy()[r, :, y0:y0 + h, x0:x0 + w].astype(np.float32)
    x = (np.arange(Wi, dtype=np.float32) + F(0.5))[None, :]
    y = (np.arange(Hi, dtype=np.float32) + F(0.5))[:, None]
    u = ((m[0] * x + m[1] * y).astype(np.float32) + m[2]).astype(np.float32)
    v = ((m[3] * x + m[4] * y).astype(np.float32) + m[5]).astype(np.float32)
    inside = (u >= 0) & (u < F(Wi)) & (v >= 0) & (v < F(Hi))
    uf = (F(Wi) - u).astype(np.float32) if flip else u

    def axis(t, n_box, n_out):
        s = np.maximum((t * (F(n_box) / F(n_out))).astype(np.float32) - F(0.5), F(0)).astype(np.float32)
        s = np.where(inside, s, F(0))
        i0 = np.minimum(s.astype(np.int64), n_box - 1)
        return i0, np.minimum(i0 + 1, n_box - 1), (s - i0.astype(np.float32)).astype(np.float32)
    ix0, ix1, fx = axis(uf, w, Wi)
    iy0, iy1, fy = axis(v, h, Hi)
    t0, t1, b0, b1 = src[:, iy0, ix0], src[:, iy0, ix1], src[:, iy1, ix0], src[:, iy1, ix1]
    t = (t0 + (fx * (t1 - t0)).astype(np.float32)).astype(np.float32)
    b = (b0 + (fx * (b1 - b0)).astype(np.float32)).astype(np.float32)
    val = (t + (fy * (b - t)).astype(np.float32)).astype(np.float32)
    fill = rw[12]
    fills = np.array([(fill >> 16) & 255, (fill >> 8) & 255, fill & 255], dtype=np.float32).reshape(3, 1, 1)
    return np.where(inside[None], val, fills).astype(np.float32)


def lut(hist, op):
    """the statistic slot's table from one channel's histogram: plain integer loops, the issue's definition"""
    h = [int(v) for v in hist]
    nz = [i for i in range(256) if h[i]]
    ident = list(range(256))
    if len(nz) < 2:
        return ident
    lo, hi = nz[0], nz[-1]
    if op == AUTOCONTRAST:
        return [0 if i < lo else max(0, min(255, (255 * (i - lo)) // (hi - lo))) for i in range(256)]
    step = (sum(h) - h[hi]) // 255
    if step == 0:
        return ident
    out, n = [], step // 2
    for i in range(256):
        out.append(min(255, n // step))
        n += h[i]
    return out


def lookup(q, rw, upto=3):
    """lookup slots [0, upto) on a quantised image q int [3,Hi,Wi] -> (q, int tables [3,256] of the statistic slot or None)"""
    rw = _words(rw)
    q = np.asarray(q).astype(np.int64)
    tables = None
    for k in range(min(3, upto)):
        op, arg = rw[2 * k], rw[2 * k + 1]
        if op == POSTERIZE:
            q = q & ~((1 << (8 - arg)) - 1)
        elif op == SOLARIZE:
            q = np.where(q < arg, q, 255 - q)
        elif op == SOLARIZE_ADD:
            q = np.where(q < 128, np.minimum(q + arg, 255), q)
        elif op == INVERT:
            q = 255 - q
        elif op in (AUTOCONTRAST, EQUALIZE):
            tables = np.array([lut(np.bincount(q[c].reshape(-1), minlength=256), op) for c in range(3)], dtype=np.int64)
            q = np.stack([tables[c][q[c]] for c in range(3)])
    return q, tables


def has_lookup(rw):
    return any(int(v) != 0 for v in _words(rw)[0:6:2])


def sample_f32(px_u8, r, box, rw, Hi, Wi):
    """(value fp32 [3,Hi,Wi] of one sample after its ra row, tables or None)"""
    v = geometry_f32(px_u8, r, box, rw, Hi, Wi)
    if not has_lookup(rw):
        return v, None
    q, tables = lookup(np.clip(np.rint(v), 0, 255).astype(np.int64), rw)
    return q.astype(np.float32), tables


def feed_f32(px_u8, rows, boxes, mix, aug, ra, Hi, Wi, mean, std):
    """the normalised fp32 image [B,3,Hi,Wi] the kernel rounds to 16 bits (const erase only: the pixel noise is not restated to the
    bit), the tables [B] and the contrast statistics [B] (None where a sample has none)"""
    B = len(rows)
    if boxes is None:
        boxes = [(0, 0, Wi, Hi, 0)] * B
    ra = [_words(r) for r in ra]
    aug = None if aug is None else [_words(a) for a in aug]
    own, tables, stats = [], [], []
    for b in range(B):
        v, t = sample_f32(px_u8, rows[b], boxes[b], ra[b], Hi, Wi)
        M = None
        if aug is not None:
            v, M = G.chain_f32(v, aug[b])
        own.append(v)
        tables.append(t)
        stats.append(M)
    out = np.empty((B, 3, Hi, Wi), dtype=np.float32)
    mean, std = np.asarray(mean, dtype=np.float32).reshape(3, 1, 1), np.asarray(std, dtype=np.float32).reshape(3, 1, 1)
    for b in range(B):
        a = own[b]
        if mix is not None:
            p, cx0, cy0, cw, ch, mb = (int(v) for v in mix[b][:6])
            m = np.array([mb], dtype=np.int32).view(np.float32)[0]
            if m != 0:
                a = fma32(m, (own[p] - a).astype(np.float32), a)
            a = a.copy()
            a[:, cy0:cy0 + ch, cx0:cx0 + cw] = own[p][:, cy0:cy0 + ch, cx0:cx0 + cw]
        n = (((a / F(255)).astype(np.float32) - mean).astype(np.float32) / std).astype(np.float32)
        if aug is not None:
            ex0, ey0, ew, eh, emode = aug[b][6:11]
            assert emode == 0 or ew == 0 or eh == 0, "the pixel-mode noise is not restated here"
            n[:, ey0:ey0 + eh, ex0:ex0 + ew] = 0
        out[b] = n
    return out, tables, stats


def patch_rows(img_f32, p, dt, keep=None):
    """[B,3,Hi,Wi] fp32 -> [B, patches (or K), 3 p p] of the 16-bit type dt (round to nearest even), as the kernel lays them out"""
    x = torch.from_numpy(np.ascontiguousarray(img_f32)).to(dt)
    B, _, Hi, Wi = x.shape
    gh, gw = Hi // p, Wi // p
    rows = x.view(B, 3, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, 3 * p * p)
    if keep is not None:
        rows = torch.stack([rows[b][torch.as_tensor(keep[b]).long()] for b in range(B)])
    return rows


# ---- the derived bound of the geometry (module docstring) ------------------------------------------------------------------------
def geometry_bound(rw, box, Hi, Wi, D):
    """(dp, e): the largest position error of u or v and the bound on |geometry_f32 - float64| for a source whose adjacent bytes differ
    by at most D"""
    rw = _words(rw)
    m = np.abs(np.array(rw[6:12], dtype=np.int64).astype(np.uint32).view(np.float32).astype(np.float64))
    _, _, w, h, _ = box
    slack = 1.0 + 2.0 ** -20
    dpx = 3 * U * (m[0] * Wi + m[1] * Hi + m[2]) * slack
    dpy = 3 * U * (m[3] * Wi + m[4] * Hi + m[5]) * slack
    dsx = (w / Wi) * (dpx + U * Wi) + 3 * U * (w + 0.5) * slack
    dsy = (h / Hi) * dpy + 3 * U * (h + 0.5) * slack
    return max(dpx, dpy), D * (dsx + dsy) + 5 * U * 255 * slack
