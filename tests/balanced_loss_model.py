"""Restatement and DERIVED bound of the class-weighted, logit-adjusted loss (cara_cross_entropy_bal: xent_bal_kernel + xent_sum_kernel,
cara_amd/csrc/norm_misc.hip), shared by tests/test_balanced_loss_model.py (host) and tests/test_balanced_loss_gpu.py (device).  In the
manner of tests/mix_model.py: a float64 value `v` per output and a term `d` counted from the roundings the kernel performs; nothing
here is fitted to a device.
"""
import torch

from oracle.small_kernels import U, gamma
from tests.mix_model import _f32, _lane_sum, f64, mix_columns

# Every first-order term below is evaluated at the exact z = l + bias, not at the fp32 z the kernel holds, and products of two error
# terms are dropped; both are of relative size u max(1, |z|) against the term they belong to.  One factor on every bound covers them
# for |z| < 2^13.
SECOND_ORDER = 1.0 + 2.0 ** -10

# the inputs the issue sets: a long-tailed count vector of 1 000 images (per class count), for any class count
def long_tail_counts(Cn, total=1000):
    """int64 [Cn]: counts falling off as 1 / (1 + c) ** 1.5 from class 0, summing to `total` where Cn allows (the head classes
    take the rounding's remainder); the tail holds ones, twos and -- from about 60 classes on -- zeros"""
    r = 1.0 / (1.0 + torch.arange(Cn, dtype=torch.float64)) ** 1.5
    n = torch.floor(r / r.sum() * total + 0.35).long()
    n[0] += total - int(n.sum())
    assert int(n.min()) >= 0 and int(n.sum()) == total
    return n


def xent_bal(logits, labels, mix, eps, cw, cb, dscale=1.0, loss_scale=1.0):
    """xent_bal_kernel + xent_sum_kernel for VALID labels, partners and weights; cw / cb fp32 [C] or None (all ones / all zeros).
        z_c = l_c + cb_c,  q as in mix_model.xent_mix,  W = sum_c cw_c q_c,  term_b = (W lse - sum_c cw_c q_c z_c) / B,
        dlogits = (p_c W - cw_c q_c) gsc,   gsc = dscale loss_scale / B.
    What is counted, beyond mix_model.xent_mix (whose rho, e_s, e_lse and weight roundings wa: 3, wb: 2, u = eps / C: 1 are kept):
    * the bias addition: one rounding, e_z,c = u |z_c| (0 without a bias).  lse is 1-Lipschitz in max_c |dz_c| and the kernel's passes
      are xent's on the rounded z:   e_lse = [xent's on z] + max_c e_z,c.
    * Sw = sum_c cw_c, lane-strided then six stages:   e_Sw = gamma(k) sum |cw_c|,  k = ceil(C / 64) + 6.
    * Swz = sum_c cw_c z_c: the product rounds once more (or not at all under an fma) and carries z's error:
          e_Swz = gamma(k + 1) sum |cw_c z_c| + sum |cw_c| e_z,c.
    * W = wa cw_ya + wb cw_yb + u Sw: the weight products (wa's three roundings and one: 4; wb: 3), their sum (5), u Sw (2, and u e_Sw)
      and the last addition (6 on the longest path):
          e_W = gamma(6) (|wa cw_ya| + |wb cw_yb| + |u Sw|) + u e_Sw.
    * dot = wa (cw_ya z_ya) + wb (cw_yb z_yb) + u Swz: as W with one more product each (cw_y z_y) and z's own error:
          e_dot = gamma(7) (|wa cw_ya z_ya| + |wb cw_yb z_yb| + |u Swz|) + |wa cw_ya| e_z,ya + |wb cw_yb| e_z,yb + u e_Swz.
    * term_b = (W lse - dot) (1 / B): the product W lse (both factors' errors and one rounding), the subtraction, the rounded 1 / B
      and the product with it:
          e_t = (|W| e_lse + |lse| e_W + u |W lse| + e_dot + 3u |W lse - dot|) / B.
      The loss is xent's tree over the terms.
    * dlogits: p = __expf(z_c - lse) knows its argument to e_lse + e_z,c + u |a'| (p (e_lse + e_z,c + rho(a'))); p W: W's error and one
      rounding; cw_c q_c: q's five (mix_model) and the product: gamma(6) |cw_c| q_c; the subtraction and the scale as in xent (6u):
          d = |gsc| (|W| p (e_lse + e_z,c + (3 |a'| + 3) u) + p e_W + u p |W| + gamma(6) |cw_c| q_c) + 6u |dlogits|
              + 2^-126 max(|gsc|, 1) max(|W|, 1).
    A fused multiply-add in place of a product and a sum removes a rounding and adds none.  Every bound is multiplied by
    SECOND_ORDER (above)."""
    l, y = f64(logits), labels.detach().cpu().long()
    B, C = l.shape
    partner, t = mix_columns(mix, B)
    e = _f32(eps)
    w = torch.ones(C, dtype=torch.float64) if cw is None else f64(cw)
    z = l if cb is None else l + f64(cb)
    e_z = torch.zeros_like(z) if cb is None else U * z.abs() + 2.0 ** -149
    ya, yb = y, y[partner]
    tc = t[:, None]
    wa, wb, u = (1 - e) * (1 - tc), (1 - e) * tc, e / C
    m = z.max(1, keepdim=True).values
    a = z - m
    ea = torch.exp(a)
    s = ea.sum(1, keepdim=True)
    k = -(-C // 64) + 6
    e_s = (ea * ((3 * a.abs() + 3) * U + gamma(k))).sum(1, keepdim=True) + C * 2.0 ** -126
    lse = m + torch.log(s)
    e_lse = e_s / s + 4 * U * torch.log(s).abs() + U * lse.abs() + e_z.max(1, keepdim=True).values
    Sw = w.sum().expand(B, 1)
    e_Sw = gamma(k) * w.abs().sum()
    Swz = (w * z).sum(1, keepdim=True)
    e_Swz = gamma(k + 1) * (w * z).abs().sum(1, keepdim=True) + (w.abs() * e_z).sum(1, keepdim=True)
    ga, gb = w[ya][:, None], w[yb][:, None]
    za, zb = z.gather(1, ya[:, None]), z.gather(1, yb[:, None])
    eza, ezb = e_z.gather(1, ya[:, None]), e_z.gather(1, yb[:, None])
    W = wa * ga + wb * gb + u * Sw
    e_W = gamma(6) * ((wa * ga).abs() + (wb * gb).abs() + (u * Sw).abs()) + u * e_Sw
    dot = wa * ga * za + wb * gb * zb + u * Swz
    e_dot = gamma(7) * ((wa * ga * za).abs() + (wb * gb * zb).abs() + (u * Swz).abs()) + (wa * ga).abs() * eza + (wb * gb).abs() * ezb + u * e_Swz
    raw = W * lse - dot
    term = (raw / B)[:, 0]
    e_t = ((W.abs() * e_lse + lse.abs() * e_W + U * (W * lse).abs() + e_dot + 3 * U * raw.abs()) / B)[:, 0] + 2.0 ** -149
    loss = term.sum()
    e_loss = e_t.sum() + gamma(-(-B // 64) + 6) * term.abs().sum()
    gsc = dscale * loss_scale / B
    ap = z - lse
    p = torch.exp(ap)
    q = torch.zeros_like(l).scatter_add_(1, ya[:, None], wa.expand(B, 1).clone()).scatter_add_(1, yb[:, None], wb.expand(B, 1).clone()) + u
    dl = (p * W - w * q) * gsc
    d = abs(gsc) * (W.abs() * p * (e_lse + e_z + (3 * ap.abs() + 3) * U) + p * e_W + U * p * W.abs() + gamma(6) * w.abs() * q) \
        + 6 * U * dl.abs() + 2.0 ** -126 * max(abs(gsc), 1.0) * W.abs().clamp_min(1.0)
    so = SECOND_ORDER
    return {"terms": (term, so * (e_t + U * term.abs())), "loss": (loss, so * (e_loss + U * loss.abs())), "dlogits": (dl, so * d), "q": q,
            "z": z, "w": w}


def xent_bal_f32(logits, labels, mix, eps, cw, cb, dscale=1.0, loss_scale=1.0):
    """the kernel's operations in its order, in torch fp32 on the host (torch's exp / log for __expf / __logf; no fused multiply-add)
    -> terms, loss, dlogits"""
    l, y = logits.float().cpu(), labels.detach().cpu().long()
    B, C = l.shape
    partner, t = mix_columns(mix, B)
    t = t.float()[:, None]
    f = lambda v: torch.tensor(v, dtype=torch.float32)   # noqa: E731
    e = f(eps)
    w = torch.ones(C, dtype=torch.float32) if cw is None else cw.float().cpu()
    z = l if cb is None else l + cb.float().cpu()
    m = z.max(1, keepdim=True).values
    sw = _lane_sum(w[None, :].expand(B, C))
    swz = _lane_sum(w * z)
    s = _lane_sum(torch.exp(z - m))
    lse = m + torch.log(s)
    ya, yb = y, y[partner]
    wa, wb, u = (f(1.0) - e) * (f(1.0) - t), (f(1.0) - e) * t, e / f(float(C))
    ga, gb = w[ya][:, None], w[yb][:, None]
    W = wa * ga + wb * gb
    if float(u) != 0.0:
        W = W + u * sw
    invB = f(1.0) / f(float(B))
    gsc = invB * f(dscale) * f(loss_scale)
    col = torch.arange(C)[None, :]
    q = torch.where(col == ya[:, None], wa, f(0.0)) + torch.where(col == yb[:, None], wb, f(0.0)) + u
    dl = (torch.exp(z - lse) * W - w * q) * gsc
    dot = wa * (ga * z.gather(1, ya[:, None])) + wb * (gb * z.gather(1, yb[:, None]))
    if float(u) != 0.0:
        dot = dot + u * swz
    term = ((W * lse - dot) * invB)[:, 0]
    return term, _lane_sum(term[None, :])[0, 0], dl


def torch_loss(logits64, q64, cw64, cb64):
    """the definition: torch.nn.functional.cross_entropy(logits + bias, q, weight = w, reduction = "sum") / B on float64 leaves ->
    (loss, d loss / d logits)"""
    import torch.nn.functional as F
    x = logits64.clone().requires_grad_(True)
    zz = x if cb64 is None else x + cb64
    loss = F.cross_entropy(zz, q64, weight=cw64, reduction="sum") / x.shape[0]
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g


# ---- the GPU test's inputs (made once per shape, on the host) --------------------------------------------------------------
BAL_C = (1, 2, 63, 64, 65, 100, 397)
BAL_B = (1, 63, 65)


def presets(Cn):
    """(class weights, logit bias) fp32 [Cn] of long_tail_counts(Cn): data.balanced_class_weight and data.logit_prior"""
    from cara_amd.data import balanced_class_weight, logit_prior
    n = long_tail_counts(Cn)
    return balanced_class_weight(n), logit_prior(n)


def bal_case(B, Cn, t, seed=0):
    """logits uniform in [-8, 8], labels uniform over the classes, partner = B - 1 - b with weight t (None: no table)"""
    g = torch.Generator().manual_seed(1000 * B + Cn + 7919 * seed)
    l = (torch.rand(B, Cn, generator=g) * 16.0 - 8.0).float()
    y = torch.randint(0, Cn, (B,), generator=g)
    if t is None:
        return l, y, None
    tb = int(torch.tensor(t, dtype=torch.float32).view(torch.int32))
    mix = torch.tensor([[B - 1 - i, 0, 0, 0, 0, 0, tb, 0] for i in range(B)], dtype=torch.int32)
    return l, y, mix


def variants():
    """every combination the issue names: (weight?, bias?) in weight only / bias only / both, with and without a mix, with and without
    smoothing; one of the scale settings each, both over the whole set -> (use_w, use_b, t, eps, (dscale, loss_scale))"""
    out = []
    for i, (use_w, use_b) in enumerate(((True, False), (False, True), (True, True))):
        for j, t in enumerate((None, 0.3)):
            for k, eps in enumerate((0.0, 0.1)):
                out.append((use_w, use_b, t, eps, (0.25, 512.0) if (i + j + k) % 2 else (1.0, 1.0)))
    return out
