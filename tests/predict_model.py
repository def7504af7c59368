"""A DERIVED fp32 error bound for the two rounded outputs of ``cara_eval_predict`` (cara_amd/csrc/eval.hip) against its fp64 host
model ``evalcount.predict_rows``, in the manner of tests/views_model.py, with the unit roundoff ``U`` and the chain bound ``gamma`` of
oracle/small_kernels.py and the same per-operation allowances:

* ``expf(a)`` with ``a`` a rounded difference:  relative ``rho(a) = (3 |a| + 3) u`` (the rounding of ``a`` moves ``exp`` by ``|a| u``;
  the rest is the allowance of the documented 1-ulp ``expf``, taken as generously as views_model takes it), results below 2^-126
  absolute 2^-126;
* ``logf(s)``:  ``4u |ln s|``;   a sum of n terms along its longest chain:  ``gamma(n)`` of the terms' magnitudes;
* every other fp32 operation one rounding, ``u |result|``;  a result below 2^-126 absolute 2^-149.

The indices and the rank depend on comparisons of fp32 values only: they have no bound, they are exact.

Per row l [C] with m = max l (exact: a maximum rounds nothing), a_c = l[c] - m <= 0:
  s = sum_c expf(a_c):  a lane adds at most 4 ceil(C / 256) <= C / 64 + 4 terms from its 16-byte loads and one from the scalar tail
      (fewer on the scalar path), wave_sum six more stages: the longest chain has at most ceil(C / 64) + 11 additions,
                                                      e_s = sum_c exp(a_c) rho(a_c) + gamma(ceil(C / 64) + 11) s + C 2^-126
  prob_j = expf(a_j) / s, the division correctly rounded: relative errors rho(a_j), e_s / s and u; each is below 2^-9 for any row
      the kernel accepts below 2^15 classes and |a| < 2^12, so the product of the three factors is inside their sum times
      SECOND = 1 + 2^-7:                              d_prob = p_j (rho(a_j) + e_s / s + u) SECOND + 2^-126 / s + 2^-149
      (an exponential flushed below 2^-126 is off by at most 2^-126 before the division; the quotient may be denormal)
  lse = m + logf(s):  |ln(s (1 + x)) - ln s| <= |x| SECOND for |x| < 2^-9,
                                                      e_lse = (e_s / s) SECOND + 4u |ln s| + u |lse|
  loss = (float)((double)lse - (double)l[y]): the difference in fp64 (2^-53, counted as u^2 |loss|), one rounding to fp32,
                                                      d_loss = e_lse + (u + u^2) |loss| + 2^-149
A slot whose exact probability is 0 (``-inf`` logit, or ``j >= classes``) must be 0 itself; NaN where the model says NaN; a loss of
+inf (the label's logit is ``-inf``) as +inf itself.  Nothing here is fitted to a device.

``emulate`` performs the stated arithmetic in fp32 on the CPU -- the lane-strided partial sums of either path, the six-stage
butterfly, the fp32 ``exp`` / ``log`` of the host -- so that a test can see the bounds hold for a real fp32 evaluation and are not
orders of magnitude above it."""
import torch

from oracle.small_kernels import U, gamma

TINY = 2.0 ** -126
SECOND = 1.0 + 2.0 ** -7


def _rho(a):
    return (3.0 * a.abs() + 3.0) * U


def bounds(logits, labels, k):
    """``logits`` fp32 [B, C], ``labels`` int64 [B] or None -> (d_prob fp64 [B, k], d_loss fp64 [B] or None): how far the kernel's
    probability and loss may lie from ``evalcount.predict_rows(logits, labels, k)`` where that is finite"""
    from cara_amd import evalcount as EC
    idx, prob, loss, _ = EC.predict_rows(logits, labels, k)
    l = logits.detach().double().cpu()
    C = l.shape[1]
    m = l.max(1, keepdim=True).values
    a = l - m
    ea = torch.exp(a)
    zero = torch.zeros_like(a)
    live = ea > 0
    s = ea.sum(1, keepdim=True)
    e_s = torch.where(live, ea * _rho(torch.where(live, a, zero)), zero).sum(1, keepdim=True) + gamma(-(-C // 64) + 11) * s + C * TINY
    picked = torch.where(idx >= 0, idx, torch.zeros_like(idx)).long()
    a_j = torch.where(idx >= 0, a.gather(1, picked), torch.full_like(prob, -float("inf")))
    fin = torch.isfinite(a_j)
    p = torch.where(fin, prob, torch.zeros_like(prob))
    d_prob = p * (_rho(torch.where(fin, a_j, torch.zeros_like(a_j))) + e_s / s + U) * SECOND + TINY / s + 2.0 ** -149
    d_prob = torch.where(fin & (prob > 0), d_prob, torch.where(fin, TINY / s + 2.0 ** -149, torch.zeros_like(d_prob)))
    if labels is None:
        return d_prob, None
    lse = (m + torch.log(s))[:, 0]
    e_lse = (e_s / s)[:, 0] * SECOND + 4 * U * torch.log(s)[:, 0].abs() + U * lse.abs()
    fl = torch.isfinite(loss)
    d_loss = e_lse + (U + U * U) * torch.where(fl, loss, torch.zeros_like(loss)).abs() + 2.0 ** -149
    return d_prob, torch.where(fl, d_loss, torch.zeros_like(d_loss))


def hold(dev, want, d):
    """-> (ok mask, worst |dev - want| / d over the finite entries): a finite ``want`` within ``d`` (exactly 0 where ``d`` is 0),
    a NaN as a NaN, an infinity as itself"""
    dev = dev.detach().double().cpu()
    fin = torch.isfinite(want)
    z = torch.zeros_like(want)
    err = torch.where(fin, (dev - torch.where(fin, want, z)).abs(), z)
    same = torch.where(torch.isnan(want), torch.isnan(dev), dev == want)
    ok = torch.where(fin, (err <= d) & torch.isfinite(dev), same)
    ratio = torch.where(fin & (d > 0), err / d.clamp_min(2.0 ** -149), z)
    return ok, float(ratio.max()) if ratio.numel() else 0.0


def _lane_sum(e, vec):
    """fp32 [C] -> the kernel's sum: lane-strided partial sums (16-byte loads over the first 4 * (C // 4) classes when ``vec``, the
    scalar tail behind them), then the xor butterfly 32, 16, ... 1"""
    C = e.shape[0]
    C4 = C // 4 if vec else 0
    lanes = torch.zeros(64, dtype=torch.float32)
    for lane in range(64):
        acc = torch.zeros((), dtype=torch.float32)
        for i in range(lane, C4, 64):
            for c in range(4 * i, 4 * i + 4):
                acc = acc + e[c]
        for c in range(4 * C4 + lane, C, 64):
            acc = acc + e[c]
        lanes[lane] = acc
    o = 32
    while o:
        lanes = lanes + lanes[torch.arange(64) ^ o]
        o >>= 1
    return lanes[0]


def emulate(logits, labels, k, vec=True):
    """the stated arithmetic in fp32 (indices from the host model: they are exact) -> (prob fp32 [B, k], loss fp32 [B])"""
    from cara_amd import evalcount as EC
    idx, _, _, _ = EC.predict_rows(logits, labels, k)
    l = logits.detach().float().cpu()
    B = l.shape[0]
    prob = torch.zeros(B, k, dtype=torch.float32)
    loss = torch.zeros(B, dtype=torch.float32)
    for b in range(B):
        m = l[b].max()
        s = _lane_sum(torch.exp(l[b] - m), vec)
        for j in range(k):
            if idx[b, j] >= 0:
                prob[b, j] = torch.exp(l[b, idx[b, j]] - m) / s
        lse = m + torch.log(s)
        loss[b] = (lse.double() - l[b, labels[b]].double()).float()
    return prob, loss
