"""A float64 value and a DERIVED fp32 error bound for every output of ``cara_eval_combine_views`` (cara_amd/csrc/eval.hip), in the
manner of oracle/small_kernels.py, whose unit roundoff ``U``, chain bound ``gamma`` and per-op allowances of the cross-entropy
(``xent``'s docstring) are used as they stand:

* ``expf(a)`` with ``a`` a rounded difference:   relative ``rho(a) = (3 |a| + 3) u``, results below 2^-126 absolute 2^-126
  (the allowance of the fast ``__expf``; the accurate ``expf`` of the kernel lies inside it);
* ``logf(s)``:   ``4u |ln s|``;        a sum of n terms along its longest chain:   ``gamma(n)`` of the terms' magnitudes;
* every other fp32 operation one rounding, ``u |result|``.

PROB, per sample s, view v, class c (eval_combine_kernel):
  pass 1   m_v exact;  s_v = sum_c expf(l_v[c] - m_v): a lane adds at most ceil(C / 64) + 4 terms (four per 16-byte load and a
           scalar tail), wave_sum six stages:      e_s = sum_c exp(a0_c) rho(a0_c) + gamma(ceil(C / 64) + 10) s_v + C 2^-126
           lse_v = m_v + logf(s_v):                e_lse = e_s / s_v + 4u |ln s_v| + u |lse_v|
  pass 2   a_v = l_v[c] - lse_v:                   e_a = e_lse + u |a_v|          (-inf - finite is exact: 0)
           M = max_v a_v (one of the computed a_v: the shift cancels, out = log sum_v exp(a_v) - log V whatever M is), so the
           a_v's errors reach the result through d out / d a_v = w_v = softmax_v(a_v):      sum_v w_v e_a(v)
           t = sum_v expf(a_v - M), V terms in order:    e_t = sum_v exp(d_v) rho(d_v) + gamma(V) t + V 2^-126,  1 <= t <= V
           r = M + logf(t):                        e_r = sum_v w_v e_a(v) + e_t / t + 4u |ln t| + u |r|
           out = r - logf(V):                      d = e_r + 4u ln V + u |out| + 2^-149
  M = -inf (the class is -inf in every view): the kernel must give -inf itself, d = 0.
LOGIT:  acc = sum_v l_v in order (V - 1 additions), out = acc / V correctly rounded:   d = gamma(V - 1) sum_v |l_v| / V + u |out| + 2^-149.

``loss_bound``: what the bound on the combined rows and the fp32 log-sum-exp of ``eval_accumulate_kernel`` (the same allowances)
leave of the mean cross-entropy.  Nothing here is fitted to a device."""
import math

import torch

from oracle.small_kernels import U, gamma

TINY = 2.0 ** -126


def _rho(a):
    return (3.0 * a.abs() + 3.0) * U


def _lse_err(l):
    """fp32 log-sum-exp of the rows of ``l`` [..., C] as both eval kernels form it -> (lse, e_lse), [..., 1]"""
    C = l.shape[-1]
    m = l.max(-1, keepdim=True).values
    a0 = l - m
    ea = torch.exp(a0)
    zero = torch.zeros_like(ea)
    s = ea.sum(-1, keepdim=True)
    e_s = torch.where(ea > 0, ea * _rho(torch.where(ea > 0, a0, zero)), zero).sum(-1, keepdim=True) \
        + gamma(-(-C // 64) + 10) * s + C * TINY
    lse = m + torch.log(s)
    return lse, e_s / s + 4 * U * torch.log(s).abs() + U * lse.abs()


def combine_bound(logits, V, mode="prob"):
    """``logits`` fp32 [S*V, C] -> (v, d), fp64 [S, C]: the exact value of every output and how far the kernel's may lie from it"""
    l = logits.detach().double().cpu()
    l = l.view(l.shape[0] // V, V, l.shape[1])
    if mode == "logit":
        v = l.sum(1) / V
        return v, gamma(max(V - 1, 1)) * l.abs().sum(1) / V + U * v.abs() + 2.0 ** -149
    lse, e_lse = _lse_err(l)
    a = l - lse
    zero = torch.zeros_like(a)
    fin = torch.isfinite(a)
    e_a = torch.where(fin, e_lse + U * torch.where(fin, a, zero).abs(), zero)
    M = a.max(1, keepdim=True).values
    dead = torch.isinf(M)                                    # -inf in every view
    dv = torch.where(fin & ~dead, a - torch.where(dead, torch.zeros_like(M), M), torch.full_like(a, -float("inf")))
    ed = torch.exp(dv)
    t = ed.sum(1, keepdim=True)
    live = ed > 0
    e_t = torch.where(live, ed * _rho(torch.where(live, dv, zero)), zero).sum(1, keepdim=True) + gamma(V) * t + V * TINY
    tt = torch.where(dead, torch.ones_like(t), t)
    w = ed / tt
    r = M + torch.log(tt)
    e_r = (w * e_a).sum(1, keepdim=True) + e_t / tt + 4 * U * torch.log(tt).abs() + U * r.abs()
    out = r - math.log(V)
    d = e_r + 4 * U * math.log(V) + U * out.abs() + 2.0 ** -149
    out = torch.where(dead, M, out)
    d = torch.where(dead, torch.zeros_like(d), d)
    return out.squeeze(1), d.squeeze(1)


def hold(dev, v, d):
    """-> (ok mask, worst |dev - v| / d over the finite outputs): a finite v within d, a -inf v as -inf itself"""
    dev = dev.detach().double().cpu()
    fin = torch.isfinite(v)
    err = torch.where(fin, (dev - torch.where(fin, v, torch.zeros_like(v))).abs(), torch.zeros_like(v))
    ok = torch.where(fin, (err <= d) & torch.isfinite(dev), dev == v)
    ratio = torch.where(fin, err / d.clamp_min(2.0 ** -149), torch.zeros_like(v))
    return ok, float(ratio.max()) if ratio.numel() else 0.0


def loss_bound(v, d, labels):
    """bound on |mean cross-entropy the device reports - the fp64 one of the rows ``v``| when the device's rows lie within ``d``
    of ``v`` [n, C]: a row's log-sum-exp moves by at most max_c d (it is 1-Lipschitz in the sup norm), its label's entry by d_y,
    the accumulate kernel's own fp32 log-sum-exp by e_lse; the differences and their sum are formed in fp64."""
    y = labels.detach().cpu().long().view(-1, 1)
    _, e_lse = _lse_err(v)
    per_row = d.max(1).values + d.gather(1, y)[:, 0] + e_lse[:, 0] * (1.0 + 4 * U)
    return float(per_row.sum()) / max(v.shape[0], 1)


def boundary_margins(v, labels):
    """per row of ``v`` [n, C]: the distance of the label's entry from the value that decides top-1 (the largest other entry) and
    from the one that decides top-5 (the fifth largest other entry; inf with fewer than six classes) -> (margin1, margin5)"""
    y = labels.detach().cpu().long().view(-1, 1)
    vy = v.gather(1, y)
    others = v.clone()
    others.scatter_(1, y, -float("inf"))
    k = min(5, v.shape[1])
    top = others.topk(k, dim=1).values
    m1 = (vy[:, 0] - top[:, 0]).abs()
    m5 = (vy[:, 0] - top[:, 4]).abs() if v.shape[1] > 5 else torch.full_like(m1, float("inf"))
    return m1, m5
