"""Restatement and DERIVED bound of the sigmoid losses (cara_sigmoid_loss: sigmoid_loss_kernel + xent_sum_kernel,
cara_amd/csrc/norm_misc.hip), shared by tests/test_sigmoid_loss_model.py (host) and tests/test_sigmoid_loss_gpu.py (device).  In the
manner of tests/balanced_loss_model.py: a float64 value `v` per output and a term `d` counted from the roundings the kernel performs;
nothing here is fitted to a device.

How the term is counted.  The kernel is written in plain operators without contraction, so every +, -, *, / is one correctly
rounded fp32 operation, and oracle.small_kernels.E -- the running error analysis the AdamW model uses -- carries a bound through
them operation by operation: operands' bounds to first order plus their product, u |v| for the result's own rounding and 2^-149 for
a subnormal one (u = oracle.small_kernels.U = 2^-24).  Where the kernel performs NO rounding (a product with 1.f or 0.f, 2 q,
max(z, 0) + L at z < 0) the model still charges one: a bound may be loose, not wrong.  Three things are not plain operations:
* e = __expf(a), a = -|z| exact: mix_model's exponential term rho(a) = (3 |a| + 3) u relative (the rounded product with log2 e, the
  1-ulp v_exp_f32; xent's also pays u |a| for a rounded difference, which is kept) and an absolute 2^-126 for a flushed result --
  that is what covers e == 0 in fp32 at |z| >= 88.8 against the float64 exp(-88.8) = 2.7e-39 and exp(-200).
* L = log1p(e) as __logf(w) (e / (w - 1)), w = fl(1 + e) in [1, 2] (e where w == 1): w - 1 is exact (Sterbenz).  With f(w) =
  ln w / (w - 1), log1p(e) = e f(1 + e) and the kernel forms e f(w): |d ln f / dw| = |1 / (w ln w) - 1 / (w - 1)| <= 1 / 2 on [1, 2]
  and |w - (1 + e)| <= 2u, so f moves by at most u relative; __logf is xent's 4u (the 1-ulp v_log_f32 and the rounded product with
  ln 2), the division and the product are one rounding each: 7u relative to L, charged as 8u.  Where w == 1, e < u and
  log1p(e) = e (1 - e / 2 + ...): u.  e's own bound enters with d log1p / de = 1 / (1 + e) <= 1.  (e_log, the plain __logf of a value
  with a bound, is used by the general power below: the bound e_w moves ln w by e_w / (w - e_w).)
* m^(g - 1) = __expf((g - 1) __logf(m)) for a g that is neither 0, 1 nor 2: both of the above in sequence, the exponential's
  argument now carrying a bound (exp(v) expm1(e_arg)), and -- m lies in [0, 1] and so does every power of it -- never more than 2.
The soft target: q_c = (wa or 0) + (wb or 0) + u is at most five plain IEEE operations on host-known fp32 inputs (eps, t), so the fp32
q the kernel holds is reproduced on the host bit for bit (soft_target_f32) and its distance from the float64 q is KNOWN, not
bounded: a one-hot target (eps == 0, t == 0 or 1) carries none, which is what keeps m = q s- + (1 - q) s+ sharp where q == 1 meets
a saturated s+; it never exceeds mix_model.xent_mix's gamma(5) q (asserted).  A thresholded q is 0 or 1 exactly -- the caller
asserts |q - thr| >= 2^-10 on the float64 q, which gamma(5) q < 2^-21 cannot cross.
Sums: a lane adds ceil(C / 64) terms, then the six stages of wave_sum: gamma(ceil(C / 64) + 6) times the sum of the terms' magnitudes
(each taken at its bound), plus the terms' own bounds; the loss is xent's tree over the samples.  invBD is the fp32 nearest to 1 / (B D): u / (B D).  gsc = invBD dscale loss_scale: two more products.
"""
import functools

import torch

from oracle.small_kernels import E, U, gamma
from tests.mix_model import _f32, _lane_sum, f64, mix_columns

TINY = 2.0 ** -126


def _where(c, a, b):
    return E(torch.where(c, a.v, b.v), torch.where(c, a.e, b.e))


def e_exp(a):
    """__expf of a value with a bound"""
    v = torch.exp(a.v)
    return E(v, v * (torch.expm1(a.e.clamp_max(700.0)) + (3 * a.v.abs() + 3) * U) + TINY)


def e_log(w):
    """__logf of a positive value with a bound (unbounded where the bound reaches the value: callers cap what they make of it)"""
    v = torch.log(w.v)
    lo = (w.v - w.e).clamp_min(1e-300)
    return E(v, w.e / lo + 4 * U * v.abs() + 2.0 ** -149)


def e_log1p(e):
    """log1p of a value in [0, 1] with a bound, as the kernel forms it (8u relative: see the module's text)"""
    v = torch.log1p(e.v)
    return E(v, e.e + 8 * U * v + 2.0 ** -149)


def soft_target(labels, mix, eps, B, Cn):
    """float64 q [B, Cn] of xent_mix_kernel (eps the fp32 the kernel gets)"""
    y = labels.detach().cpu().long()
    partner, t = mix_columns(mix, B)
    e = _f32(eps)
    ya, yb = y, y[partner]
    wa, wb, u = ((1 - e) * (1 - t))[:, None], ((1 - e) * t)[:, None], e / Cn
    return torch.zeros(B, Cn, dtype=torch.float64).scatter_add_(1, ya[:, None], wa.expand(B, 1).clone()).scatter_add_(1, yb[:, None], wb.expand(B, 1).clone()) + u


def soft_target_f32(labels, mix, eps, B, Cn):
    """fp32 q [B, Cn] in the kernel's operations and order (plain IEEE: the same bits on any machine)"""
    y = labels.detach().cpu().long()
    partner, t = mix_columns(mix, B)
    t = t.float()[:, None]
    f = lambda v: torch.tensor(v, dtype=torch.float32)   # noqa: E731
    e_ = f(eps)
    ya, yb = y, y[partner]
    col = torch.arange(Cn)[None, :]
    wa, wb, u = (f(1.0) - e_) * (f(1.0) - t), (f(1.0) - e_) * t, e_ / f(float(Cn))
    return torch.where(col == ya[:, None], wa, f(0.0)) + torch.where(col == yb[:, None], wb, f(0.0)) + u


def margin(q, thr):
    """how far the float64 target stays from the threshold (the tests assert >= 2^-10 before they threshold)"""
    return float((q - float(_f32(thr))).abs().min())


def sigmoid_loss(logits, labels, mix, eps, thr=None, fgamma=0.0, alpha=None, pw=None, sum_classes=False, dscale=1.0, loss_scale=1.0):
    """sigmoid_loss_kernel + xent_sum_kernel for VALID labels, partners and weights -> {"terms", "loss", "dlogits": (v, d), "q"}.
    thr / alpha None: none; pw fp32 [C] or None (BCE only).  The operations are the kernel's, in its order (see the kernel's comment):
        e = __expf(-|z|), w = 1 + e, L = log1p(e) [= __logf(w) (e / (w - 1))], r = 1 / w, er = e r;  s+ / s- = r / er in the order of z's sign;
        sp(z) = max(z, 0) + L, sp(-z) = max(-z, 0) + L;  omq = 1 - q;
        BCE:    pq = pw q,  l = pq sp(-z) + omq sp(z),  g = omq s+ - pq s-;
        focal:  ce = q sp(-z) + omq sp(z),  m = q s- + omq s+,  d0 = omq s+ - q s-,  mg1 = m^(g - 1),  mg = mg1 m,
                l = mg ce,  g = d0 mg + g ce mg1 (s+ s-) (1 - 2 q)   [g == 0: l = ce, g = d0],
                a = alpha q + (1 - alpha) omq:  l = a l,  g = a g;
        term_b = (sum_c l) invBD,  dlogits = g gsc."""
    z = f64(logits)
    B, Cn = z.shape
    q64 = soft_target(labels, mix, eps, B, Cn)
    if thr is None:
        e_q = (soft_target_f32(labels, mix, eps, B, Cn).double() - q64).abs()
        assert bool((e_q <= gamma(5) * q64).all())
        q = E(q64, e_q)
    else:
        q = E((q64 > float(_f32(thr))).double())
    one = E(1.0)
    focal = fgamma > 0 or alpha is not None
    assert not (focal and pw is not None)
    e = e_exp(E(-z.abs()))
    w = one + e
    L = e_log1p(e)
    r = one / w
    er = e * r
    pos = z >= 0
    sp, sm = _where(pos, r, er), _where(pos, er, r)
    spz, spn = E(z.clamp_min(0.0)) + L, E((-z).clamp_min(0.0)) + L
    omq = one - q
    if not focal:
        pq = E(torch.ones(Cn, dtype=torch.float64) if pw is None else f64(pw)) * q
        l = pq * spn + omq * spz
        g = omq * sp - pq * sm
    else:
        ce = q * spn + omq * spz
        m = q * sm + omq * sp
        d0 = omq * sp - q * sm
        fg = float(_f32(fgamma))
        if fg == 0.0:
            l, g = ce, d0
        else:
            if fg == 1.0:
                mg1 = E(torch.ones_like(z))
            elif fg == 2.0:
                mg1 = m
            else:
                mg1 = e_exp((one * (fg - 1.0)) * e_log(m))          # (g - 1 is one rounded subtraction: one * charges it)
                mg1 = E(mg1.v, mg1.e.clamp_max(2.0))
            mg = mg1 * m
            l = mg * ce
            g = d0 * mg + E(fg) * ce * mg1 * (sp * sm) * (one - E(2.0) * q)
        if alpha is not None:
            al = E(float(_f32(alpha)))
            a = al * q + (one - al) * omq
            l, g = a * l, a * g
    k = -(-Cn // 64) + 6
    S = E(l.v.sum(1), l.e.sum(1) + gamma(k) * (l.v.abs() + l.e).sum(1))
    D = 1 if sum_classes else Cn
    invBD = E(1.0 / (B * D), torch.tensor(U / (B * D), dtype=torch.float64))
    term = S * invBD
    loss = term.v.sum()
    e_loss = term.e.sum() + gamma(-(-B // 64) + 6) * (term.v.abs() + term.e).sum() + U * abs(loss) + 2.0 ** -149
    gsc = invBD * E(float(_f32(dscale))) * E(float(_f32(loss_scale)))
    dl = g * gsc
    return {"terms": (term.v, term.e), "loss": (loss, e_loss), "dlogits": (dl.v, dl.e), "q": q64}


# ---- the definitions, on float64 leaves ---------------------------------------------------------------------------------------
def torch_bce(logits64, q64, pw64, sum_classes):
    """torch.nn.functional.binary_cross_entropy_with_logits(z, q, pos_weight = pw), "mean" (or "sum" / B) -> (loss, d loss / d z)"""
    import torch.nn.functional as F
    x = logits64.clone().requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(x, q64, pos_weight=pw64, reduction="sum") / (x.shape[0] * (1 if sum_classes else x.shape[1]))
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g


def written_focal(logits64, q64, fgamma, alpha, sum_classes):
    """the focal loss as the header writes it -- p = sigmoid(z), ce = BCE(z, q), m = q (1 - p) + (1 - q) p, a m^gamma ce -- through
    autograd -> (loss, d loss / d z).  (torchvision's sigmoid_focal_loss writes 1 - p_t, p_t = p q + (1 - p)(1 - q): the same m.)"""
    import torch.nn.functional as F
    x = logits64.clone().requires_grad_(True)
    p = torch.sigmoid(x)
    ce = F.binary_cross_entropy_with_logits(x, q64, reduction="none")
    m = q64 * torch.sigmoid(-x) + (1 - q64) * p
    l = ce * (m ** fgamma if fgamma else 1.0)
    if alpha is not None:
        l = (alpha * q64 + (1 - alpha) * (1 - q64)) * l
    loss = l.sum() / (x.shape[0] * (1 if sum_classes else x.shape[1]))
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g


# ---- the kernel's operations in fp32 on the host, and six ways to get them wrong ---------------------------------------------
SLIPS = ("naive_softplus", "divisor_B", "pos_weight_on_negative", "no_1_minus_2q", "m_as_p_plus_q_minus_2pq", "threshold_before_smoothing")


def sigmoid_loss_f32(logits, labels, mix, eps, thr=None, fgamma=0.0, alpha=None, pw=None, sum_classes=False, dscale=1.0, loss_scale=1.0,
                     slip=None):
    """the kernel's operations in its order, in torch fp32 on the host (torch's exp / log for __expf / __logf; no fused multiply-add)
    -> terms, loss, dlogits.  ``slip``: one of SLIPS, the mistake made on purpose."""
    z, y = logits.float().cpu(), labels.detach().cpu().long()
    B, Cn = z.shape
    partner, t = mix_columns(mix, B)
    t = t.float()[:, None]
    f = lambda v: torch.tensor(v, dtype=torch.float32)   # noqa: E731
    e_ = f(eps)
    ya, yb = y, y[partner]
    col = torch.arange(Cn)[None, :]
    if slip == "threshold_before_smoothing" and thr is not None:
        hard = torch.where(col == ya[:, None], f(1.0) - t, f(0.0)) + torch.where(col == yb[:, None], t, f(0.0))
        hard = torch.where(hard > f(thr), f(1.0), f(0.0))
        q = (f(1.0) - e_) * hard + e_ / f(float(Cn))
    else:
        q = soft_target_f32(labels, mix, eps, B, Cn)
        if thr is not None:
            q = torch.where(q > f(thr), f(1.0), f(0.0))
    omq = f(1.0) - q
    e = torch.exp(-z.abs())
    w = f(1.0) + e
    r = f(1.0) / w
    L = torch.where(w == 1.0, e, torch.log(w) * (e / (w - f(1.0)).clamp_min(2.0 ** -23)))
    er = e * r
    pos = z >= 0
    sp, sm = torch.where(pos, r, er), torch.where(pos, er, r)
    if slip == "naive_softplus":
        spz, spn = torch.log(f(1.0) + torch.exp(z)), torch.log(f(1.0) + torch.exp(-z))
    else:
        spz, spn = z.clamp_min(0.0) + L, (-z).clamp_min(0.0) + L
    focal = fgamma > 0 or alpha is not None
    if not focal:
        pwv = torch.ones(Cn) if pw is None else pw.float().cpu()
        if slip == "pos_weight_on_negative":
            l = q * spn + (pwv * omq) * spz
            g = (pwv * omq) * sp - q * sm
        else:
            pq = pwv * q
            l = pq * spn + omq * spz
            g = omq * sp - pq * sm
    else:
        ce = q * spn + omq * spz
        m = sp + q - f(2.0) * sp * q if slip == "m_as_p_plus_q_minus_2pq" else q * sm + omq * sp
        d0 = omq * sp - q * sm
        fg = f(fgamma)
        if float(fg) == 0.0:
            l, g = ce, d0
        else:
            mg1 = torch.ones_like(z) if float(fg) == 1.0 else m if float(fg) == 2.0 else torch.exp((fg - f(1.0)) * torch.log(m))
            mg = mg1 * m
            l = mg * ce
            last = f(1.0) if slip == "no_1_minus_2q" else f(1.0) - f(2.0) * q
            g = d0 * mg + fg * ce * mg1 * (sp * sm) * last
        if alpha is not None:
            a = f(alpha) * q + (f(1.0) - f(alpha)) * omq
            l, g = a * l, a * g
    D = 1 if (sum_classes or slip == "divisor_B") else Cn
    invBD = torch.tensor(1.0 / (B * D), dtype=torch.float64).float()
    gsc = invBD * f(dscale) * f(loss_scale)
    term = (_lane_sum(l) * invBD)[:, 0]
    return term, _lane_sum(term[None, :])[0, 0], g * gsc


# ---- the tests' inputs (made once per shape, on the host) ------------------------------------------------------------------------
SIG_B = (1, 3, 64, 65)                                   # the edges of the sum tree
SIG_C = (1, 2, 63, 64, 65, 100, 397, 1000)               # the lane-stride edges and the head sizes in use
PLANTED = (0.0, 2.0 ** -20, -2.0 ** -20, 17.0, -17.0, 88.8, -88.8, 200.0, -200.0)
THR = 0.2
SCALED = (0.125, 1024.0)


@functools.lru_cache(maxsize=None)
def sig_case(B, Cn, seed=0):
    """logits N(0, 3) with PLANTED on and beside every sample's label (row b: the label's column holds PLANTED[(b + seed) % 9], the
    next columns the values after it, as far as the row reaches), labels uniform, and a table with partner = B - 1 - b (a
    self-partner in the middle of an odd batch) and t cycling through 0.3, 0, 1, 0 -- a period prime to the planted values', so that
    every planted label meets a hard and a soft target -> (logits, labels, mix).  Left unchanged."""
    g = torch.Generator().manual_seed(100003 * B + 17 * Cn + 7919 * seed)
    l = (torch.randn(B, Cn, generator=g) * 3.0).float()
    y = torch.randint(0, Cn, (B,), generator=g)
    for b in range(B):
        for j in range(min(Cn, len(PLANTED))):
            l[b, (int(y[b]) + j) % Cn] = PLANTED[(b + seed + j) % len(PLANTED)]
    assert float(l.abs().max()) < 2.0 ** 13
    ts = (0.3, 0.0, 1.0, 0.0)
    bits = [int(torch.tensor(v, dtype=torch.float32).view(torch.int32)) for v in ts]
    mix = torch.tensor([[B - 1 - i, 0, 0, 0, 0, 0, bits[i % len(ts)], 0] for i in range(B)], dtype=torch.int32)
    return l, y, mix


@functools.lru_cache(maxsize=None)
def pos_weight(Cn):
    """U(0.5, 4) per class"""
    return (torch.rand(Cn, generator=torch.Generator().manual_seed(31 + Cn)) * 3.5 + 0.5).float()


# (table?, eps, thr, pos_weight: None / "ones" / "u", gamma, alpha, sum_classes, (dscale, loss_scale)): every mode the issue names,
# each setting of a column beside at least two settings of every other
VARIANTS = (
    (False, 0.0, None, None, 0.0, None, False, (1.0, 1.0)),          # torch's plain "mean" BCE
    (True, 0.1, None, "u", 0.0, None, False, SCALED),
    (True, 0.1, THR, None, 0.0, None, True, (1.0, 1.0)),             # timm's --bce-loss --bce-target-thresh 0.2 with sum_classes
    (False, 0.1, THR, "u", 0.0, None, False, (0.125, 1.0)),
    (True, 0.0, None, "ones", 0.0, None, True, (1.0, 1024.0)),
    (True, 0.0, None, "u", 0.0, None, True, (1.0, 1.0)),
    (False, 0.0, None, None, 2.0, 0.25, True, (1.0, 1.0)),           # torchvision's defaults
    (True, 0.1, None, None, 2.0, 0.25, False, SCALED),
    (True, 0.0, None, None, 1.0, None, True, (1.0, 1.0)),
    (False, 0.1, THR, None, 1.0, 0.25, False, (0.125, 1.0)),
    (True, 0.1, None, None, 0.0, 0.25, True, (1.0, 1.0)),            # alpha alone: the focal launch at gamma == 0
    (True, 0.1, THR, None, 2.0, None, True, (1.0, 1024.0)),
    (True, 0.1, None, None, 1.5, 0.25, True, (1.0, 1.0)),            # a gamma that takes the exp / log power
    (True, 0.0, None, None, 2.0, None, False, SCALED),
)


def variant_args(B, Cn, v, seed=0):
    """-> (logits, labels, mix or None, kwargs of sigmoid_loss / sigmoid_loss_f32) of VARIANTS[v]; asserts the threshold's margin"""
    table, eps, thr, pwk, fg, alpha, sumc, (dscale, ls) = VARIANTS[v]
    l, y, mix = sig_case(B, Cn, seed)
    mix = mix if table else None
    if thr is not None:
        assert margin(soft_target(y, mix, eps, B, Cn), thr) >= 2.0 ** -10
    pw = None if pwk is None else torch.ones(Cn) if pwk == "ones" else pos_weight(Cn)
    return l, y, mix, dict(eps=eps, thr=thr, fgamma=fg, alpha=alpha, pw=pw, sum_classes=sumc, dscale=dscale, loss_scale=ls)


@functools.lru_cache(maxsize=None)
def variant_model(B, Cn, v, seed=0):
    """the float64 values and bounds of one case, computed once and shared by both operand builds (left unchanged)"""
    l, y, mix, kw = variant_args(B, Cn, v, seed)
    return sigmoid_loss(l, y, mix, **kw)
