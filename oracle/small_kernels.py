"""Plain float64 restatements of the kernels AROUND the blocks -- the LayerNorm family, the fp32 head, cross-entropy, AdamW
(cara_amd/csrc/norm_misc.hip, vit.hip's head kernels, optim.hip) -- each with a bound DERIVED from the kernel's arithmetic.

Every restatement returns, per output, the float64 value `v` the kernel would give with exact fp32 arithmetic (rounded to a
16-bit operand exactly where the kernel rounds, and nowhere else) and a per-element term `d`: how far the kernel's fp32 value can
lie from `v`, counted from the roundings the kernel performs.  u = 2^-24 is the unit roundoff of fp32, gamma(n) = n u / (1 - n u)
the standard bound of n roundings in a chain (Higham, Accuracy and Stability of Numerical Algorithms, 3.1).  Nothing here is
fitted to a device: tests/test_small_kernels_model.py proves on the host that an fp32 restatement in ANOTHER summation order
stays inside every bound and that ten plausible slips do not; tests/test_small_kernels_gpu.py then holds the device to it.

The two rules (hold_f32, hold_16):
* an fp32 output w is held to |w - v| <= d, element by element;
* a 16-bit output w is held to "w == round16(v), or w is the 16-bit NEIGHBOUR of round16(v) on the side where v lies within d of
  the rounding boundary": rounding is monotone, so a true fp32 value inside [v - d, v + d] rounds into
  [round16(v - d), round16(v + d)].  Where d is below a 16-bit step -- everywhere but on rows whose |mean| dwarfs their spread --
  that interval IS "the model's value or its neighbour"; on such an offset row (mean 100, spread 1e-2: the mean's fp32 error times
  rstd = 100 is itself a bf16 step of y) the interval is the rule, and an fp32 evaluation in another order does land two steps
  away there.  Elements that differ from round16(v) are counted as neighbour cases; every test caps their share.
"""
import math

import torch

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def f64(t):
    return t.detach().double().cpu()


def round16(v, dt):
    """what the kernels' (bf16)f / (_Float16)f conversion gives for the fp32 nearest to v"""
    return v.float().to(dt)


def _ordinal(t):
    """16-bit floats as integers in value order (sign-magnitude -> two's complement); +0 and -0 coincide"""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def hold_f32(dev, v, d):
    """-> (ok mask, worst |dev - v| / d).  d > 0 everywhere (each term carries its own final rounding u |v| and a denormal)."""
    err = (f64(dev) - v).abs()
    ok = err <= d
    ok &= torch.isfinite(f64(dev))
    return ok, float((err / d).max()) if err.numel() else 0.0


def hold_16(dev, v, d, dt):
    """-> (ok mask, neighbour mask, worst |dev - v| / (d + half a 16-bit step))"""
    dev = dev.detach().cpu()
    model, lo, hi = round16(v, dt), round16(v - d, dt), round16(v + d, dt)
    od, om = _ordinal(dev), _ordinal(model)
    neighbour = od != om
    ok = (od >= _ordinal(lo)) & (od <= _ordinal(hi)) & torch.isfinite(dev.double())
    step = (model.double().abs() * 2.0 ** (-7 if dt == torch.bfloat16 else -10)).clamp_min(2.0 ** -24)   # >= one 16-bit step
    ratio = (dev.double() - v).abs() / (d + 0.5 * step)
    return ok, neighbour, float(ratio.max()) if ratio.numel() else 0.0


# ----------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------------------------------------------------------
def kappa_ln(C):
    """Roundings on the longest path of ln_fwd_kernel's / ln_bwd_kernel's row sums (norm_misc.hip: `s += (x + y) + (z + w)` over
    V4 = C / 256 float4 per lane, then wave_sum's six __shfl_xor stages, common.h): at most 4 V4 in-lane adds plus six."""
    return 4 * (C // 256) + 6


def kappa_head(D):
    """head_fwd_f32_kernel (vit.hip): a thread adds ceil(D / 256) elements, wave_sum six stages, `(red[0] + red[1]) + (red[2] +
    red[3])` two more."""
    return -(-D // 256) + 6 + 2


def ln_fwd(x, g, b, eps, kappa=None):
    """y = (x - mu) rstd gamma + beta of one row per wave (ln_fwd_kernel, norm_misc.hip lines `const float mu = wave_sum(s) *
    (1.0f / C)` ... `bf16x4 o = {...}`).  x [M, C] float64-convertible; returns dict of (v, d) pairs for mean, rstd, y.

    mean.  s is a tree of kappa roundings over the x_i, then one product with the rounded constant 1/C:
        |mu^ - mu| <= gamma(kappa + 2) mean|x_i| =: e_mu.        (mean|x_i| >= |mu|: THE conditioning term of an offset row)
    rstd.  The kernel's second pass is the two-pass variance about mu^ = mu + e:  sum (x_i - mu^)^2 = sum (x_i - mu)^2 + C e^2
        exactly, so var^ = (var + e^2)(1 + gamma(kappa + 5)) [subtract 1, square 2 incl. the operand, tree kappa, 1/C 2], the
        addition of eps one more rounding, and rsqrtf at most 1 ulp = 2u (ROCm device math: rsqrtf 1 ULP):
        r = (gamma(kappa + 6)(var + e_mu^2 + eps) + e_mu^2) / (var + eps),   |rstd^ - rstd| <= rstd (r / 2 + r^2 + 2u) =: e_rs.
        On a constant row var = 0 and everything rests on eps: r = e_mu^2 / eps, which is why e_mu must be in the bound.
    y.  t = x_i - mu^ carries e_mu + u |x_i - mu|; times rstd^ (e_rs, u), times gamma_i (u), plus beta_i (u |y|); a contracted
        fma only removes roundings:
        d_y = |gamma_i| rstd (e_mu + u |x_i - mu|) + |xhat_i gamma_i| (e_rs / rstd + 3u) + 2u |y_i|.
        The first term is the one that grows with |mu| rstd |gamma|."""
    x, g, b = f64(x), f64(g), f64(b)
    C = x.shape[1]
    k = kappa_ln(C) if kappa is None else kappa
    mu = x.mean(1, keepdim=True)
    e_mu = gamma(k + 2) * x.abs().mean(1, keepdim=True) + 2.0 ** -149
    xc = x - mu
    var = (xc * xc).mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + eps)
    r = (gamma(k + 6) * (var + e_mu ** 2 + eps) + e_mu ** 2) / (var + eps)
    e_rs = rs * (r / 2 + r * r + 2 * U)
    xh = xc * rs
    y = xh * g + b
    d_y = g.abs() * rs * (e_mu + U * xc.abs()) + (xh * g).abs() * (e_rs / rs + 3 * U) + 2 * U * y.abs() + 2.0 ** -149
    return {"mean": (mu[:, 0], e_mu[:, 0] + U * mu[:, 0].abs()), "rstd": (rs[:, 0], e_rs[:, 0] + U * rs[:, 0]), "y": (y, d_y)}


def ln_bwd(dy, x, g, mean, rstd, dx_in=None, rowscale=None, rows_per_sample=1, kappa=None):
    """dx = rstd (gh - c1 - xhat c2) [+ dx_in],  gh = dy gamma, c1 = mean(gh), c2 = mean(gh xhat), and dyb = dx * rowscale[row /
    rows_per_sample] (ln_bwd_kernel, norm_misc.hip).  mean and rstd are the fp32 values the forward LEFT: inputs, taken as exact.

    xhat_i = (x_i - mean) rstd: 2 roundings.  gh_i = dy_i gamma_i: 1.  s1 is the tree over gh, s2 over gh_i xhat_i (product: the
    two operands' 3 roundings + 1), each times the rounded 1/C (2):
        e_c1 = gamma(kappa + 3) mean|gh|,   e_c2 = gamma(kappa + 6) mean|gh xhat|.
    Inside the bracket: gh_i (u), c1 (e_c1), xhat_i c2 (|xhat| e_c2 + 3u |xhat c2|), two subtractions (2u of the magnitudes);
    the product with rstd (u) and the addition of dx_in (u):
        d_dx = rstd (e_c1 + |xhat_i| e_c2 + 3u (|gh_i| + |c1|) + 5u |xhat_i c2|) + u |o_i| + u |o_i + dx_in_i|.
    dyb = (16-bit)(dx^ sc): d_dyb = |sc| d_dx + u |dx sc|."""
    dy, x, g, mean, rstd = f64(dy), f64(x), f64(g), f64(mean)[:, None], f64(rstd)[:, None]
    M, C = x.shape
    k = kappa_ln(C) if kappa is None else kappa
    xh = (x - mean) * rstd
    gh = dy * g
    c1, c2 = gh.mean(1, keepdim=True), (gh * xh).mean(1, keepdim=True)
    e_c1, e_c2 = gamma(k + 3) * gh.abs().mean(1, keepdim=True), gamma(k + 6) * (gh * xh).abs().mean(1, keepdim=True)
    o = rstd * (gh - c1 - xh * c2)
    d = rstd * (e_c1 + xh.abs() * e_c2 + 3 * U * (gh.abs() + c1.abs()) + 5 * U * (xh * c2).abs()) + U * o.abs() + 2.0 ** -149
    dx = o if dx_in is None else o + f64(dx_in)
    d = d + U * dx.abs()
    sc = torch.ones(M, 1, dtype=torch.float64) if rowscale is None else f64(rowscale)[torch.arange(M) // rows_per_sample][:, None]
    dyb = dx * sc
    return {"dx": (dx, d), "dyb": (dyb, sc.abs() * d + U * dyb.abs() + 2.0 ** -149)}


def kappa_xu(C):
    """Roundings on the longest path of block_contract's sums (norm_misc.hip): a wave chains V4 = C / 256 MFMA steps
    `acc = mfma_f32_16x16x32(a, u, acc)` -- each adds 32 products to the accumulator, in an order the hardware does not state: at
    most 32 roundings per step -- and `t += L.part[w]` adds the eight waves' partial tiles in sequence (7): 32 V4 + 7."""
    return 32 * (C // 256) + 7


def xu_contract(y16, Ut):
    """T = (16-bit)(y U^T) of the fused kernels (block_contract, norm_misc.hip): y16 [M, C] are the 16-bit rows the kernel staged
    in LDS (its own output y, resp. dyb), Ut [Rp, C] the packed 16-bit factor: inputs, taken as exact.  A product of two 16-bit
    values is exact in fp32 (bf16: 16 significand bits, fp16: 22), so only the additions round:
        d_T = gamma(kappa_xu(C)) sum_k |y_k u_k|.
    Columns whose factor rows are zero (beyond the rank) come out as exact zeros."""
    y, u = f64(y16), f64(Ut)
    return {"T": (y @ u.t(), gamma(kappa_xu(y.shape[1])) * (y.abs() @ u.abs().t()) + 2.0 ** -149)}


# ----------------------------------------------------------------------------------------------------------------------------
# The head
# ----------------------------------------------------------------------------------------------------------------------------
def head_fwd(x, g, b, W, hb, eps):
    """head_fwd_f32_kernel (vit.hip): LayerNorm of the cls row in fp32 with the kernel's own tree (kappa_head; the mean and the
    variance are DIVIDED by D: one rounding instead of two, covered), xn kept in fp32 for the products and rounded once to 16 bits
    for the backward, logits_c = sum_d W[c, d] xn[d] + hb[c].
    A lane adds ceil(D / 256) float4 dot pieces of depth 3, then six shuffle stages; each product one rounding; the bias one:
        d_logit = gamma(3 ceil(D / 256) + 7) sum_d |W xn| + sum_d |W| d_xn + u |logit|."""
    D = x.shape[1]
    ln = ln_fwd(x, g, b, eps, kappa=kappa_head(D))
    xn, d_xn = ln["y"]
    W, hb = f64(W), f64(hb)
    logits = xn @ W.t() + hb
    d = gamma(3 * -(-D // 256) + 7) * (xn.abs() @ W.abs().t()) + d_xn @ W.abs().t() + U * logits.abs() + 2.0 ** -149
    return {"mean": ln["mean"], "rstd": ln["rstd"], "xn16": (xn, d_xn), "logits": (logits, d)}


def head_bwd(dl, xn16, W):
    """head_bwd_kernel (vit.hip): three plain loops, a product and an addition per term (or one fma), n terms in sequence:
        dW[c, d] = sum_b dl[b, c] xn[b, d]     d = gamma(B) sum |.|         db[c] = sum_b dl[b, c]     d = gamma(B - 1) sum |.|
        dxn[b, d] = (16-bit) sum_c dl[b, c] W[c, d]     d = gamma(classes) sum |.|"""
    dl, xn, W = f64(dl), f64(xn16), f64(W)
    B, Cn = dl.shape
    tiny = 2.0 ** -149
    return {"dW": (dl.t() @ xn, gamma(B) * (dl.abs().t() @ xn.abs()) + tiny),
            "db": (dl.sum(0), gamma(max(B - 1, 1)) * dl.abs().sum(0) + tiny),
            "dxn": (dl @ W, gamma(Cn) * (dl.abs() @ W.abs()) + tiny)}


# ----------------------------------------------------------------------------------------------------------------------------
# Cross-entropy
# ----------------------------------------------------------------------------------------------------------------------------
def xent(logits, labels, dscale=1.0, loss_scale=1.0):
    """xent_kernel + xent_sum_kernel (norm_misc.hip): one wave per sample, m = max, s = sum __expf(l_c - m), lse = m + __logf(s),
    term_b = (lse - l_y) / B, loss = sum_b term_b, dlogits = (__expf(l_c - lse) - [c == y]) (1/B) dscale loss_scale.
    A label outside [0, classes) makes that sample's term and its dlogits row NaN (and so the loss).

    __expf(a) is v_exp_f32(a log2(e)): the product with the rounded constant moves the exponent by 2u |a| log2(e), i.e. the
    result by 2u |a| relative, and v_exp_f32 is good to 1 ulp = 2u (CDNA ISA guide); a itself is a rounded difference (u |a|);
    results below 2^-126 are flushed (absolute 2^-126):            rho(a) = (3 |a| + 3) u.
    s: a lane adds ceil(C / 64) terms, then six stages: e_s = sum_c exp(a_c) (rho(a_c) + gamma(ceil(C / 64) + 6)).
    __logf(s) = v_log_f32(s) ln 2: 1 ulp and a product with a rounded constant: 4u |ln s|; the addition to m one rounding:
        e_lse = e_s / s + 4u |ln s| + u |lse|.
    term_b: the subtraction, the rounded 1/B and the product: e_t = (e_lse + 3u |lse - l_y|) / B; the loss is a tree of
    ceil(B / 64) + 6 roundings over the terms.
    dlogits: p = __expf(a'), a' = l_c - lse known to e_lse + u |a'|: p (e_lse + rho(a')); the subtraction u; the scale is three
    products of rounded values (4u):     d = |gsc| p (e_lse + (3 |a'| + 3) u) + 6u |dlogits| + 2^-126 |gsc|."""
    l, y = f64(logits), labels.detach().cpu().long()
    B, C = l.shape
    ok = (y >= 0) & (y < C)
    ys = torch.where(ok, y, torch.zeros_like(y))
    m = l.max(1, keepdim=True).values
    a = l - m
    ea = torch.exp(a)
    s = ea.sum(1, keepdim=True)
    e_s = (ea * ((3 * a.abs() + 3) * U + gamma(-(-C // 64) + 6))).sum(1, keepdim=True) + C * 2.0 ** -126
    lse = m + torch.log(s)
    e_lse = e_s / s + 4 * U * torch.log(s).abs() + U * lse.abs()
    ly = l.gather(1, ys[:, None])
    term = (lse - ly)[:, 0] / B
    e_t = (e_lse[:, 0] + 3 * U * (lse - ly)[:, 0].abs()) / B + 2.0 ** -149
    nan = float("nan")
    term = torch.where(ok, term, torch.full_like(term, nan))
    loss = term.sum()
    e_loss = e_t.sum() + gamma(-(-B // 64) + 6) * term.abs().sum()
    gsc = dscale * loss_scale / B
    ap = l - lse
    p = torch.exp(ap)
    onehot = torch.zeros_like(l).scatter_(1, ys[:, None], 1.0)
    dl = (p - onehot) * gsc
    d = abs(gsc) * p * (e_lse + (3 * ap.abs() + 3) * U) + 6 * U * dl.abs() + 2.0 ** -126 * max(abs(gsc), 1.0)
    dl = torch.where(ok[:, None], dl, torch.full_like(dl, nan))
    return {"terms": (term, e_t + U * term.abs()), "loss": (loss, e_loss + U * loss.abs()), "dlogits": (dl, d)}


# ----------------------------------------------------------------------------------------------------------------------------
# AdamW: a running error analysis, operation by operation
# ----------------------------------------------------------------------------------------------------------------------------
class E:
    """A float64 value with a bound on how far the fp32 computation of it can be away: every operation propagates its operands'
    bounds to first order and adds its own correctly rounded result's u |v| (hipcc's default keeps fp32 division and sqrtf
    correctly rounded; `extra` adds the ulps of a function that is not)."""

    def __init__(self, v, e=None):
        self.v = v if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float64)
        self.e = torch.zeros_like(self.v) if e is None else e

    @staticmethod
    def lift(o):
        return o if isinstance(o, E) else E(o)

    def _r(self, v, e):
        return E(v, e + U * v.abs() + 2.0 ** -149)

    def __add__(self, o):
        o = E.lift(o)
        return self._r(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = E.lift(o)
        return self._r(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = E.lift(o)
        return self._r(self.v * o.v, self.e * o.v.abs() + o.e * self.v.abs() + self.e * o.e)

    def __truediv__(self, o):
        o = E.lift(o)
        q = self.v / o.v
        lo = (o.v.abs() - o.e).clamp_min(2.0 ** -149)
        return self._r(q, self.e / lo + q.abs() * o.e / lo)

    def sqrt(self):
        v = torch.sqrt(self.v)
        # |sqrt(a + e) - sqrt(a)| <= e / sqrt(a) for e <= a, and <= sqrt(e) always
        return self._r(v, torch.minimum(self.e / v.clamp_min(2.0 ** -149), torch.sqrt(self.e)))


def f32(v):
    """a host double as the fp32 the argument struct carries"""
    return torch.tensor(float(v), dtype=torch.float32).double()


def adamw(p, g, m, v, *, lr, wd, beta1, beta2, eps, step, dyn=False, rounding=True):
    """One adamw_kernel step (optim.hip) on fp32 tensors, every line of the kernel as one E operation:
        decay = 1 - lr wd;  p *= decay;  m += (1 - beta1)(g - m);  v = beta2 v + (1 - beta2) g g;
        p -= (lr / bc1) (m / (sqrt(v) / bc2s + eps)).
    The host form gets bc1 = 1 - beta1^t and bc2s = sqrt(1 - beta2^t) as fp32 arguments computed in double (cara_amd/optim.py):
    exact inputs.  The dyn form computes them in the kernel: bc1 = 1 - powf(1 - one_minus_beta1, t), bc2s = sqrtf(1 -
    powf(beta2, t)) -- the base 1 - one_minus_beta1 is one rounding, which the power multiplies by t; powf is good to 1 ulp = 2u
    (ROCm device math: powf 1 ULP): e_pow = b^t (t e_b / b + 2u).  Both forms are held to the SAME values: bc from the double
    betas as the host computes them, the dyn form's extra term being the distance of its fp32 route from that.
    rounding = False: plain float64 of the same formulas (equals torch.optim.AdamW in float64)."""
    if not rounding:
        p, g, m, v = (t.double() for t in (p, g, m, v))
        p = p * (1 - lr * wd)
        m = m + (1 - beta1) * (g - m)
        v = beta2 * v + (1 - beta2) * g * g
        p = p - (lr / (1 - beta1 ** step)) * (m / (v.sqrt() / math.sqrt(1 - beta2 ** step) + eps))
        return {"p": (p, None), "m": (m, None), "v": (v, None)}
    P, G, M, V = (E(f64(t)) for t in (p, g, m, v))
    omb1, b2, omb2, lr_, wd_, eps_ = (E(f32(c)) for c in (1.0 - beta1, beta2, 1.0 - beta2, lr, wd, eps))
    if dyn:
        base = E(1.0) - omb1
        pw = base.v ** step
        bc1 = E(1.0) - E(pw, pw * (step * base.e / base.v + 2 * U))
        pw2 = b2.v ** step
        bc2s = (E(1.0) - E(pw2, pw2 * 2 * U)).sqrt()
        # held to the host's double-precision corrections: move the centre there, keep the distance in the bound
        h1, h2 = 1.0 - beta1 ** step, math.sqrt(1.0 - beta2 ** step)
        bc1 = E(torch.tensor(h1, dtype=torch.float64), bc1.e + (bc1.v - h1).abs())
        bc2s = E(torch.tensor(h2, dtype=torch.float64), bc2s.e + (bc2s.v - h2).abs())
    else:
        bc1, bc2s = E(f32(1.0 - beta1 ** step)), E(f32(math.sqrt(1.0 - beta2 ** step)))
    decay = E(1.0) - lr_ * wd_
    step_size = lr_ / bc1
    pi = P * decay
    mi = M + omb1 * (G - M)
    vi = b2 * V + omb2 * G * G
    denom = vi.sqrt() / bc2s + eps_
    pi = pi - step_size * (mi / denom)
    return {"p": (pi.v, pi.e), "m": (mi.v, mi.e), "v": (vi.v, vi.e)}
