"""Restatements and DERIVED bounds of the mixed resident feed (cara_im2col_patches_u8_rows_mix, cara_cross_entropy_mix), shared by
tests/test_mix_model.py (host) and tests/test_mix_gpu.py (device).  In the manner of oracle/small_kernels.py: a float64 value `v` per
output and a term `d` counted from the roundings the kernel performs; nothing here is fitted to a device.
"""
import torch

from oracle.small_kernels import U, gamma

IMAGENET_STD_MIN = 0.224

# ---- patch rows ------------------------------------------------------------------------------------------------------------
# The crop test's bound (tests/test_augmented_feed_gpu.py, test_scaled_boxes_...): an unmixed element of these shapes (source
# 40 x 52, positions s < 52) is off by less than 7.1e-3 of a byte step from the fp32 evaluation of the sample position and the
# lerps, i.e. by less than E_CROP = 1.3e-4 after (v / 255 - mean) / std with std >= 0.224 (7.1e-3 / 255 / 0.224 = 1.243e-4; the
# rest is the three roundings of the normalisation of |x| < 2.7, 5e-7).
E_CROP = 1.3e-4
# The blend v = a + m (b - a), 0 <= m <= 1, of two such values on the 0..255 scale: the inputs' errors enter as (1 - m) da + m db
# <= max(da, db) -- no more than one unmixed element's -- and the blend adds the rounding of b - a (u |b - a| <= 255 u) and those
# of the product and the sum (an fma: one; separately: two, each of a value <= 255): at most 3 x 255 u on the byte scale, that is
# 3 u / std after normalisation.
E_MIX = E_CROP + 3 * U / IMAGENET_STD_MIN


# ---- the loss --------------------------------------------------------------------------------------------------------------
# The loss bars of a whole train step against the fp32 oracle, relative to max(1, |loss|): the figures
# tests/test_model_gpu.py::test_train_step_against_oracle holds (bf16 5e-3, fp16 5e-4), named here once for the mixed step
LOSS_BAR = {"bf16": 5.0e-3, "fp16": 5.0e-4}


def f64(t):
    return t.detach().double().cpu()


def _f32(v):
    return torch.tensor(float(v), dtype=torch.float32).double()


def mix_columns(mix, B):
    """(partner int64 [B], t float64 [B]) of a table, or the identity's for None"""
    if mix is None:
        return torch.arange(B), torch.zeros(B, dtype=torch.float64)
    mix = mix.detach().cpu().to(torch.int32).contiguous()
    return mix[:, 0].long(), mix[:, 6].contiguous().view(torch.float32).double()


def xent_mix(logits, labels, mix, eps, dscale=1.0, loss_scale=1.0):
    """xent_mix_kernel + xent_sum_kernel (norm_misc.hip) for VALID labels, partners and weights: oracle.small_kernels.xent with the
    soft target q_c = wa [c == ya] + wb [c == yb] + u,  wa = (1 - eps)(1 - t), wb = (1 - eps) t, u = eps / C.  eps and t are fp32
    inputs (exact).  Up to lse everything is xent's (same passes):
        rho(a) = (3 |a| + 3) u,  e_s = sum_c exp(a_c) (rho(a_c) + gamma(ceil(C / 64) + 6)),  e_lse = e_s / s + 4u |ln s| + u |lse|.
    The new reduction S = sum_c l_c: a lane adds ceil(C / 64) terms, then six shuffle stages:   e_S = gamma(ceil(C / 64) + 6) sum|l_c|.
    The weights: 1 - eps, 1 - t and their product round (wa: 3), wb: 2 (1 - eps, the product), u: 1 (the division; C is exact).
    dot = (1 - eps) (l_ya + t (l_yb - l_ya)) + u S (the lerp is exact at t == 0 and where ya == yb): the difference, its product
    with t, the sum, 1 - eps, the product with it and the last addition -- six roundings on the longest path, of values bounded
    by (1 - eps) (|l_ya| + t |l_yb - l_ya|) and |u S|; S enters with its own error times u:
        e_dot = gamma(6) ((1 - eps) (|l_ya| + t |l_yb - l_ya|) + |u S|) + u e_S.
    term_b = (lse - dot) (1 / B): the subtraction, the rounded 1 / B and the product:   e_t = (e_lse + e_dot + 3u |lse - dot|) / B.
    The loss is xent's tree over the terms.
    dlogits = (p - q) gsc with p = __expf(l_c - lse) as in xent (p (e_lse + rho(a'))) and q_c = (wa or 0) + (wb or 0) + u: wa's
    three roundings and the two additions, all terms >= 0, so |q^ - q| <= gamma(5) q:
        d = |gsc| (p (e_lse + (3 |a'| + 3) u) + gamma(5) q) + 6u |dlogits| + 2^-126 max(|gsc|, 1).
    With eps == 0 and t == 0 this is xent's bound plus nothing (wa == 1 and q == the one-hot exactly; gamma(5) q stays in: a
    bound may be loose, not wrong)."""
    l, y = f64(logits), labels.detach().cpu().long()
    B, C = l.shape
    partner, t = mix_columns(mix, B)
    e = _f32(eps)
    ya, yb = y, y[partner]
    wa, wb, u = ((1 - e) * (1 - t))[:, None], ((1 - e) * t)[:, None], e / C
    m = l.max(1, keepdim=True).values
    a = l - m
    ea = torch.exp(a)
    s = ea.sum(1, keepdim=True)
    k = -(-C // 64) + 6
    e_s = (ea * ((3 * a.abs() + 3) * U + gamma(k))).sum(1, keepdim=True) + C * 2.0 ** -126
    lse = m + torch.log(s)
    e_lse = e_s / s + 4 * U * torch.log(s).abs() + U * lse.abs()
    S = l.sum(1, keepdim=True)
    e_S = gamma(k) * l.abs().sum(1, keepdim=True)
    lya, lyb = l.gather(1, ya[:, None]), l.gather(1, yb[:, None])
    tc = t[:, None]
    dot = (1 - e) * (lya + tc * (lyb - lya)) + u * S
    e_dot = gamma(6) * ((1 - e) * (lya.abs() + tc * (lyb - lya).abs()) + (u * S).abs()) + u * e_S
    term = ((lse - dot) / B)[:, 0]
    e_t = ((e_lse + e_dot + 3 * U * (lse - dot).abs()) / B)[:, 0] + 2.0 ** -149
    loss = term.sum()
    e_loss = e_t.sum() + gamma(-(-B // 64) + 6) * term.abs().sum()
    gsc = dscale * loss_scale / B
    ap = l - lse
    p = torch.exp(ap)
    q = torch.zeros_like(l).scatter_add_(1, ya[:, None], wa.expand(B, 1).clone()).scatter_add_(1, yb[:, None], wb.expand(B, 1).clone()) + u
    dl = (p - q) * gsc
    d = abs(gsc) * (p * (e_lse + (3 * ap.abs() + 3) * U) + gamma(5) * q) + 6 * U * dl.abs() + 2.0 ** -126 * max(abs(gsc), 1.0)
    return {"terms": (term, e_t + U * term.abs()), "loss": (loss, e_loss + U * loss.abs()), "dlogits": (dl, d), "q": q}


def _lane_sum(t):
    """fp32 row sums in the kernel's order: lane i adds elements i, i + 64, ... in sequence, then the butterfly of wave_sum (lanes
    32, 16, 8, 4, 2, 1 apart: common.h)"""
    B, C = t.shape
    k = -(-C // 64)
    pad = torch.zeros(B, k * 64, dtype=torch.float32)
    pad[:, :C] = t
    pad = pad.view(B, k, 64)
    acc = torch.zeros(B, 64, dtype=torch.float32)
    for j in range(k):
        acc = acc + pad[:, j]
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, torch.arange(64) ^ off]
    return acc[:, :1]


def xent_mix_f32(logits, labels, mix, eps, dscale=1.0, loss_scale=1.0):
    """the kernel's operations in its order, in torch fp32 on the host (torch's exp / log for __expf / __logf) -> terms, loss, dlogits"""
    l, y = logits.float().cpu(), labels.detach().cpu().long()
    B, C = l.shape
    partner, t = mix_columns(mix, B)
    t = t.float()[:, None]
    f = lambda v: torch.tensor(v, dtype=torch.float32)   # noqa: E731
    e = f(eps)
    m = l.max(1, keepdim=True).values
    sl = _lane_sum(l)
    s = _lane_sum(torch.exp(l - m))
    lse = m + torch.log(s)
    ya, yb = y, y[partner]
    wa, wb, u = (f(1.0) - e) * (f(1.0) - t), (f(1.0) - e) * t, e / f(float(C))
    invB = f(1.0) / f(float(B))
    gsc = invB * f(dscale) * f(loss_scale)
    col = torch.arange(C)[None, :]
    q = torch.where(col == ya[:, None], wa, f(0.0)) + torch.where(col == yb[:, None], wb, f(0.0)) + u
    dl = (torch.exp(l - lse) - q) * gsc
    la = l.gather(1, ya[:, None])
    dot = (f(1.0) - e) * (la + t * (l.gather(1, yb[:, None]) - la))
    if float(u) != 0.0:
        dot = dot + u * sl
    term = ((lse - dot) * invB)[:, 0]
    return term, _lane_sum(term[None, :])[0, 0], dl


def loss_case(B, Cn, t, same):
    """tests.small_kernels_common.xent_inputs' logits (spread up to +-80, a repeated maximum, all equal) and labels (on the maximum /
    the minimum), with partner = B - 1 - b and weight t: the partner's label equal to the sample's (same) or another class"""
    from tests.small_kernels_common import xent_inputs
    l, y = xent_inputs(B, Cn)
    i = torch.arange(B)
    partner = B - 1 - i
    if same or Cn == 1:
        y = y[torch.minimum(i, partner)]          # a pair shares its label
    else:
        y = torch.where(i < (B + 1) // 2, y, (y[partner] + 1 + i) % Cn)
    tb = int(torch.tensor(t, dtype=torch.float32).view(torch.int32))
    mix = torch.tensor([[int(p), 0, 0, 0, 0, 0, tb, 0] for p in partner], dtype=torch.int32)
    return l, y, mix
