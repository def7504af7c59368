"""Restatement and DERIVED bound of the distillation loss (cara_distill_loss: distill_kernel + xent_sum_kernel,
cara_amd/csrc/norm_misc.hip), shared by tests/test_distill_model.py (host) and tests/test_distill_gpu.py (device).  In the manner of
tests/sigmoid_loss_model.py: a float64 value `v` per output and a term `d` counted from the roundings the kernel performs; nothing
here is fitted to a device.

How the term is counted.  The kernel is written in plain operators without contraction, so every +, -, *, / is one correctly
rounded fp32 operation and oracle.small_kernels.E carries a bound through them operation by operation (operands' bounds to first
order plus their product, u |v| for the result's own rounding, 2^-149 for a subnormal one).  Where the kernel performs NO rounding
(x * 1.f at T == 1, 0.f * x at alpha == 1, T * T at a power of two) the model still charges one: a bound may be loose, not wrong.
What is not a plain operation is taken from tests/sigmoid_loss_model.py and tests/mix_model.py:
* __expf of a value with a bound (e_exp): relative (3 |a| + 3) u plus what the argument's bound does to it, absolute 2^-126 for a
  flushed result;  __logf of a positive value with a bound (e_log): 4u |ln| plus the argument's relative bound.
* a lane sum of ceil(C / 64) terms and six butterfly stages: gamma(ceil(C / 64) + 6) times the sum of the terms' magnitudes (each at
  its bound) plus the terms' own bounds; the loss is the same tree over the samples.
* the soft target q is reproduced on the host bit for bit (soft_target_f32): its distance from the float64 q is known, not bounded.
New here:
* invT = 1 / T: one division of two exact fp32 values;  x invT: one product per element (the tempered logit x / T as the kernel
  forms it: 2u |x / T| from the true quotient);  aT = a T and aT2 = aT T: one product each.
* tempered_lse(x, invT) = m + __logf(sum_c __expf(x_c invT - m)), m = max_c x_c invT: the maximum selects, it does not round, so m is
  off by no more than the largest bound of the row's products; the difference, the exponential, the lane sum, the logarithm and the
  addition follow as E operations.  (m's own error cancels in the true lse; the running analysis counts it twice: loose.)
* the KL form chosen: kl = sum_c r_c (lt_c - lz_c) with lz_c = z_c invT - lse(z / T), lt_c = t_c invT - lse(t / T), pT = __expf(lz),
  r = __expf(lt) -- the log-ratio form.  Its terms are E operations on lz and lt; its error is gamma-small relative to
  sum_c r_c (|lt_c| + |lz_c|), the teacher's entropy plus the cross-entropy, whatever the offset of either row.  The candidate
  lse(z / T) - lse(t / T) + sum_c r_c (t_c - z_c) / T instead carries u (|lse(z / T)| + |lse(t / T)|), which grows with the rows'
  offsets (60 at |z| = 30, T = 0.5) while the KL itself does not, and it is not exactly 0 for equal rows.
* hard mode: yt = the first index of the teacher row's maximum, taken on the same fp32 values on both sides: exact.
"""
import functools

import torch

from oracle.small_kernels import E, U, gamma
from tests.mix_model import _f32, _lane_sum, f64, mix_columns
from tests.sigmoid_loss_model import e_exp, e_log, soft_target, soft_target_f32


def _rows(e):
    """E of a [B, C] value -> E of the row sums as the kernel's lane sum forms them, [B, 1]"""
    k = -(-e.v.shape[1] // 64) + 6
    return E(e.v.sum(1, keepdim=True), e.e.sum(1, keepdim=True) + gamma(k) * (e.v.abs() + e.e).sum(1, keepdim=True))


def tempered_lse(x, invT):
    """tempered_lse of norm_misc.hip on a float64 [B, C] of exact fp32 values and invT an E -> (E of x invT, E of the lse [B, 1])"""
    a = E(x) * invT
    idx = a.v.argmax(1, keepdim=True)
    m = E(a.v.gather(1, idx), a.e.max(1, keepdim=True).values)
    s = _rows(e_exp(a - m))
    return a, m + e_log(s)


def distill_loss(logits, teacher, labels, mix, eps, alpha, temperature=1.0, hard=False, dscale=1.0, loss_scale=1.0):
    """distill_kernel + xent_sum_kernel for VALID labels, partners, weights and a finite teacher, alpha > 0
    -> {"terms", "loss", "dlogits": (v, d), "q", "yt"}.  The operations are the kernel's, in its order (see the kernel's comment)."""
    z, t = f64(logits), f64(teacher)
    B, Cn = z.shape
    y = labels.detach().cpu().long()
    partner, tm = mix_columns(mix, B)
    q64 = soft_target(labels, mix, eps, B, Cn)
    e_q = (soft_target_f32(labels, mix, eps, B, Cn).double() - q64).abs()
    assert bool((e_q <= gamma(5) * q64).all())
    q = E(q64, e_q)
    one = E(1.0)
    al, ep = E(float(_f32(alpha))), E(float(_f32(eps)))
    oma = one - al
    # the cross-entropy's part: sl, lse, dot (xent_mix_kernel's forms)
    k = -(-Cn // 64) + 6
    sl = E(z.sum(1, keepdim=True), gamma(k) * z.abs().sum(1, keepdim=True))
    _, lse = tempered_lse(z, one)
    la, lb = z.gather(1, y[:, None]), z.gather(1, y[partner][:, None])
    dot = (one - ep) * (E(la) + E(tm[:, None]) * (E(lb) - E(la)))
    if float(_f32(eps)) != 0.0:
        dot = dot + (ep / E(float(Cn))) * sl
    invB = one / E(float(B))
    gsc = invB * E(float(_f32(dscale))) * E(float(_f32(loss_scale)))
    p = e_exp(E(z) - lse)
    if hard:
        yt = t.argmax(1)                              # (the first of equal maxima: torch's rule and the kernel's)
        col = torch.arange(Cn)[None, :]
        at = E(torch.where(col == yt[:, None], al.v, torch.zeros((), dtype=torch.float64)))
        qd = oma * q + at
        g = (p - qd) * gsc
        term = (lse - (oma * dot + al * E(z.gather(1, yt[:, None])))) * invB
    else:
        yt = None
        T = E(float(_f32(temperature)))
        invT = one / T
        aT = al * T
        aT2 = aT * T
        az, lseZ = tempered_lse(z, invT)
        at_, lseT = tempered_lse(t, invT)
        lz, lt = az - lseZ, at_ - lseT
        pT, r = e_exp(lz), e_exp(lt)
        kl = _rows(r * (lt - lz))
        g = (oma * (p - q) + aT * (pT - r)) * gsc
        term = (oma * (lse - dot) + aT2 * kl) * invB
    term = E(term.v[:, 0], term.e[:, 0])
    loss = term.v.sum()
    e_loss = term.e.sum() + gamma(-(-B // 64) + 6) * (term.v.abs() + term.e).sum() + U * abs(loss) + 2.0 ** -149
    return {"terms": (term.v, term.e), "loss": (loss, e_loss), "dlogits": (g.v, g.e), "q": q64, "yt": yt}


# ---- the definition, on float64 leaves ---------------------------------------------------------------------------------------------
def torch_distill(logits64, teacher64, q64, alpha, temperature, hard):
    """the issue's formula through torch and autograd -> (loss, d loss / d z): soft
    (1 - a) cross_entropy(z, q) + a T^2 kl_div(log_softmax(z / T), softmax(t / T), reduction="batchmean"); hard: cross_entropy(z, q')"""
    import torch.nn.functional as F
    x = logits64.clone().requires_grad_(True)
    if hard:
        qd = (1 - alpha) * q64 + alpha * F.one_hot(teacher64.argmax(1), x.shape[1]).double()
        loss = F.cross_entropy(x, qd)
    else:
        T = temperature
        loss = (1 - alpha) * F.cross_entropy(x, q64) + alpha * T * T * F.kl_div(F.log_softmax(x / T, 1), F.softmax(teacher64 / T, 1),
                                                                                reduction="batchmean")
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g


# ---- the kernel's operations in fp32 on the host, and seven ways to get them wrong -------------------------------------------------
SLIPS = ("no_T2_in_loss", "no_T_in_grad", "kl_reversed", "teacher_at_T1", "alpha_on_wrong_term", "yt_from_student", "divisor_BC")


def _lse_f32(x, invT):
    a = x * invT
    m = a.max(1, keepdim=True).values
    return a, m + torch.log(_lane_sum(torch.exp(a - m)))


def distill_loss_f32(logits, teacher, labels, mix, eps, alpha, temperature=1.0, hard=False, dscale=1.0, loss_scale=1.0, slip=None):
    """the kernel's operations in its order, in torch fp32 on the host (torch's exp / log for __expf / __logf; no fused multiply-add)
    -> terms, loss, dlogits.  ``slip``: one of SLIPS, the mistake made on purpose."""
    z, t, y = logits.float().cpu(), teacher.float().cpu(), labels.detach().cpu().long()
    B, Cn = z.shape
    partner, tm = mix_columns(mix, B)
    tm = tm.float()[:, None]
    f = lambda v: torch.tensor(v, dtype=torch.float32)   # noqa: E731
    e_, al = f(eps), f(alpha)
    oma = f(1.0) - al
    if slip == "alpha_on_wrong_term":
        al, oma = oma, al
    q = soft_target_f32(labels, mix, eps, B, Cn)
    sl = _lane_sum(z)
    _, lse = _lse_f32(z, f(1.0))
    la = z.gather(1, y[:, None])
    dot = (f(1.0) - e_) * (la + tm * (z.gather(1, y[partner][:, None]) - la))
    u = e_ / f(float(Cn))
    if float(u) != 0.0:
        dot = dot + u * sl
    invB = f(1.0) / f(float(B * Cn if slip == "divisor_BC" else B))
    gsc = invB * f(dscale) * f(loss_scale)
    p = torch.exp(z - lse)
    if hard:
        yt = (z if slip == "yt_from_student" else t).argmax(1)
        col = torch.arange(Cn)[None, :]
        qd = oma * q + torch.where(col == yt[:, None], al, f(0.0))
        g = (p - qd) * gsc
        term = (lse - (oma * dot + al * z.gather(1, yt[:, None]))) * invB
    else:
        T = f(temperature)
        invT = f(1.0) / T
        aT = al * T
        aT2 = aT * T
        az, lseZ = _lse_f32(z, invT)
        at_, lseT = _lse_f32(t, f(1.0) if slip == "teacher_at_T1" else invT)
        lz, lt = az - lseZ, at_ - lseT
        pT, r = torch.exp(lz), torch.exp(lt)
        kl = _lane_sum(pT * (lz - lt)) if slip == "kl_reversed" else _lane_sum(r * (lt - lz))
        g = (oma * (p - q) + (al if slip == "no_T_in_grad" else aT) * (pT - r)) * gsc
        term = (oma * (lse - dot) + (al if slip == "no_T2_in_loss" else aT2) * kl) * invB
    term = term[:, 0]
    return term, _lane_sum(term[None, :])[0, 0], g


# ---- the tests' inputs (made once per shape, on the host) ----------------------------------------------------------------------------
KD_B = (1, 3, 64, 65)                                    # the edges of the sum tree
KD_C = (1, 2, 63, 64, 65, 100, 397, 1000)                # the lane-stride edges and the head sizes in use
PEAK = 30.0                                              # |z| up to 30: z / T reaches 60 at T = 0.5
SCALED = (0.5, 1024.0)


@functools.lru_cache(maxsize=None)
def kd_case(B, Cn, peaked, seed=0):
    """student logits, teacher logits, labels and a table -> (z, t, y, mix).  Flat: N(0, 1).  Peaked: N(0, 10) clamped to +-PEAK with
    +PEAK planted on the label and -PEAK beside it.  The teacher is the student's row shrunk and disturbed (0.7 z + noise of the same
    spread, clamped alike) -- a teacher that mostly agrees -- and every third row holds its maximum TWICE (the tie rule of hard mode).
    The table: partner = b + 1 (mod B), never b itself where B > 1, t = 0.3.  Left unchanged."""
    g = torch.Generator().manual_seed(7 + 100003 * B + 17 * Cn + 7919 * seed + (1 if peaked else 0))
    spread = 10.0 if peaked else 1.0
    z = (torch.randn(B, Cn, generator=g) * spread).float()
    y = torch.randint(0, Cn, (B,), generator=g)
    t = (0.7 * z + 0.5 * spread * torch.randn(B, Cn, generator=g)).float()
    if peaked:
        z, t = z.clamp(-PEAK, PEAK), t.clamp(-PEAK, PEAK)
        for b in range(B):
            z[b, int(y[b])] = PEAK
            z[b, (int(y[b]) + 1) % Cn] = -PEAK if Cn > 1 else PEAK
    for b in range(0, B, 3):
        if Cn >= 2:
            hi = float(t[b].max()) if not peaked else PEAK
            t[b, (5 * b + 2) % Cn] = hi
            t[b, (5 * b + 1) % Cn] = hi
    bits = int(torch.tensor(0.3, dtype=torch.float32).view(torch.int32))
    mix = torch.tensor([[(i + 1) % B, 0, 0, 0, 0, 0, bits, 0] for i in range(B)], dtype=torch.int32)
    return z, t, y, mix


# (alpha, T, hard, table and eps = 0.1?, peaked?, scaled?): every (alpha, T) of the issue and both hard modes, each beside both
# settings of every other column
VARIANTS = (
    (0.5, 0.5, False, False, False, False), (0.5, 0.5, False, True, True, True),
    (0.5, 1.0, False, True, False, True), (0.5, 1.0, False, False, True, False),
    (0.5, 4.0, False, False, True, True), (0.5, 4.0, False, True, False, False),
    (1.0, 0.5, False, True, True, False), (1.0, 0.5, False, False, False, True),
    (1.0, 1.0, False, False, True, True), (1.0, 1.0, False, True, False, False),
    (1.0, 4.0, False, True, True, True), (1.0, 4.0, False, False, False, False),
    (0.5, 1.0, True, False, False, True), (0.5, 1.0, True, True, True, False),
    (1.0, 1.0, True, True, False, True), (1.0, 1.0, True, False, True, False),
)


def variant_args(B, Cn, v, seed=0):
    """-> (logits, teacher, labels, mix or None, kwargs of distill_loss / distill_loss_f32) of VARIANTS[v]"""
    alpha, T, hard, table, peaked, scaled = VARIANTS[v]
    z, t, y, mix = kd_case(B, Cn, peaked, seed)
    dscale, ls = SCALED if scaled else (1.0, 1.0)
    return z, t, y, (mix if table else None), dict(eps=0.1 if table else 0.0, alpha=alpha, temperature=T, hard=hard, dscale=dscale,
                                                   loss_scale=ls)


@functools.lru_cache(maxsize=None)
def variant_model(B, Cn, v, seed=0):
    """the float64 values and bounds of one case, computed once and shared by both operand builds (left unchanged)"""
    z, t, y, mix, kw = variant_args(B, Cn, v, seed)
    return distill_loss(z, t, y, mix, **kw)
