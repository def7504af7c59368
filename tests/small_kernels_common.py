"""Cases, fp32 other-order restatements and check helpers shared by tests/test_small_kernels_model.py (host),
tests/test_small_kernels_gpu.py and the older LayerNorm / head / cross-entropy tests of tests/test_kernels_gpu.py (device).  The
float64 restatements and their derived bounds are in oracle/small_kernels.py; the caps on neighbour cases in tests/tolerances.py."""
import math

import torch

from oracle import small_kernels as K

EPS = 1e-6
LN_C = [256, 768, 1024]
LN_M_FUSED = [1, 3, 4, 5, 15, 16, 17, 33]
LN_M_PLAIN = [1, 3, 4, 5, 9]
FAMILIES = ["gaussian", "offset", "constant", "outlier", "tiny", "zero"]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def family_rows(M, C, seed=0):
    """[M, C] fp32, row i of family (i + M) % 6 (so that M = 1, 3 ... meet different ones), all in one tensor: Gaussian; offset
    (mu = 100, spread 1e-2); constant; one outlier channel of 300 among O(1); tiny (1e-4 randn: eps matters); all zero"""
    g = _gen(1000 * seed + 7 * M + C)
    x = torch.randn(M, C, generator=g)
    fam = [(i + M) % 6 for i in range(M)]
    for i, f in enumerate(fam):
        if f == 1:
            x[i] = 100.0 + 1e-2 * x[i]
        elif f == 2:
            x[i] = 3.0
        elif f == 3:
            x[i, (17 * i + 5) % C] = 300.0
        elif f == 4:
            x[i] = 1e-4 * x[i]
        elif f == 5:
            x[i] = 0.0
    return x, fam


def ln_params(C, seed=0):
    g = _gen(50 + seed + C)
    return 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


def ln_bwd_inputs(M, C, dt, rps, seed=0):
    """dy (16-bit), dx_in, and a row scale that takes 0, 1 and 1 / (1 - p) (p = 0.1) inside one launch"""
    g = _gen(90 + seed + M + C)
    dy = torch.randn(M, C, generator=g).to(dt)
    dx_in = torch.randn(M, C, generator=g)
    n = (M + rps - 1) // rps
    rs = torch.tensor([0.0, 1.0, 1.0 / 0.9])[(torch.arange(n) + 1) % 3]
    return dy, dx_in, rs


# --- fp32 restatements in another order, with the slips ---------------------------------------------------------------------
def tree_sum(t, lanes=64):
    """fp32 row sums: `lanes` lanes own CONTIGUOUS runs of the row and add them last to first, then adjacent lanes pair up -- the
    kernels' depth (run + log2 lanes), none of their partial sums"""
    M, C = t.shape[0], t.shape[-1]
    t = t.reshape(*t.shape[:-1], lanes, C // lanes) if C >= lanes else t.reshape(*t.shape[:-1], C, 1)
    acc = t[..., -1]
    for j in range(t.shape[-1] - 2, -1, -1):
        acc = acc + t[..., j]
    while acc.shape[-1] > 1:
        if acc.shape[-1] % 2:
            acc = torch.cat((acc, torch.zeros_like(acc[..., :1])), -1)
        acc = acc[..., 0::2] + acc[..., 1::2]
    return acc[..., 0]


def ln_fwd_f32(x, g, b, dt, slip=None, lanes=64):
    x, g, b = x.float(), g.float(), b.float()
    C = x.shape[1]
    inv = torch.tensor(1.0 / C, dtype=torch.float32)
    mu = tree_sum(x, lanes) * inv
    if slip == "one_pass":
        var = tree_sum(x * x, lanes) * inv - mu * mu
    else:
        a = x - mu[:, None]
        var = tree_sum(a * a, lanes) * (torch.tensor(1.0 / (C - 1), dtype=torch.float32) if slip == "var_c_minus_1" else inv)
    rs = torch.rsqrt(var + (0.0 if slip == "no_eps" else torch.tensor(EPS, dtype=torch.float32)))
    if slip == "rstd_1e-4":
        rs = rs * torch.tensor(1.0001, dtype=torch.float32)
    y = (x - mu[:, None]) * rs[:, None] * g + b
    return mu, rs, y, y.to(dt)


def ln_bwd_f32(dy, x, g, mean, rstd, dx_in, rs, rps, dt, slip=None):
    x, g, dy = x.float(), g.float(), dy.float()
    M, C = x.shape
    inv = torch.tensor(1.0 / C, dtype=torch.float32)
    xh = (x - mean[:, None]) * rstd[:, None]
    gh = dy * g
    c1, c2 = tree_sum(gh) * inv, tree_sum(gh * xh) * inv
    if slip == "no_c2":
        c2 = torch.zeros_like(c2)
    o = rstd[:, None] * (gh - c1[:, None] - xh * c2[:, None])
    if dx_in is not None:
        o = o + dx_in.float()
    sc = rs.float()[torch.arange(M) // (rps + 1 if slip == "rowscale_rps_plus_1" else rps)][:, None] if rs is not None else 1.0
    return o, (o * sc).to(dt)


def xent_f32(l, y, dscale=1.0, ls=1.0, slip=None):
    l = l.float()
    B, C = l.shape
    m = l.max(1, keepdim=True).values
    s = torch.exp(l - m).flip(1).sum(1, keepdim=True)
    lse = m + torch.log(s)
    term = (lse - l.gather(1, y[:, None]))[:, 0] * torch.tensor(1.0 / B, dtype=torch.float32)
    gsc = torch.tensor(1.0 / ((B + 1) if slip == "B_plus_1" else B), dtype=torch.float32) * torch.tensor(dscale, dtype=torch.float32) * \
        torch.tensor(ls, dtype=torch.float32)
    onehot = torch.zeros_like(l).scatter_(1, y[:, None], 1.0)
    return term, term.flip(0).sum(), (torch.exp(l - lse) - onehot) * gsc


def head_bwd_f32(dl, xn16, W, dt, slip=None):
    dl, xn, W = dl.float(), xn16.float(), W.float()
    dlb = dl[:-1] if slip == "db_B_minus_1" and dl.shape[0] > 1 else dl
    return dl.flip(0).t() @ xn.flip(0), dlb.flip(0).sum(0), (dl.flip(1) @ W.flip(0)).to(dt)


def adamw_f32(p, g, m, v, *, lr, wd, beta1, beta2, eps, step, slip=None):
    """fp32, elementwise: there is no summation to reorder, so the products are associated the other way -- (1 - beta2)(g g) for the
    kernel's ((1 - beta2) g) g, (step_size m) / denom for step_size (m / denom).  The first moment keeps the kernel's lerp: its
    textbook form beta1 m + (1 - beta1) g rounds 1 - (1 - beta1) once more and IS outside the lerp's bound (1.4 x)."""
    f = lambda c: torch.tensor(c, dtype=torch.float32)  # noqa: E731
    t = step - 1 if slip == "t_minus_1" else step
    bc1, bc2s = f(1.0 - beta1 ** t), f(math.sqrt(1.0 - beta2 ** t))
    decay = f(1.0) - f(lr) * f(wd)
    m2 = m + f(1.0 - beta1) * (g - m)
    v2 = f(beta2) * v + f(1.0 - beta2) * (g * g)
    upd = ((f(lr) / bc1) * m2) / (v2.sqrt() / bc2s + f(eps))
    p2 = (p - upd) * decay if slip == "decay_after" else p * decay - upd
    return p2, m2, v2


# --- the device cases --------------------------------------------------------------------------------------------------------
HEAD_FWD_CASES = [(64, 100, 768, 197), (2, 21843, 768, 197), (3, 10, 1024, 5), (1, 257, 256, 1)]
HEAD_BWD_CASES = [(1, 1, 256), (3, 10, 1024), (5, 257, 768), (64, 100, 768)]
XENT_C = [1, 2, 63, 64, 65, 1000]
XENT_B = [1, 5]
ADAMW_SIZES = [1, 255, 256, 1023, 1024, 1025]
ADAMW_STEPS = [1, 1000]
ADAMW_HYPER = dict(lr=1e-3, wd=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)


def head_fwd_inputs(B, classes, D):
    x, fam = family_rows(B, D, seed=3)
    g = _gen(B + classes + D)
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    W, hb = 0.02 * torch.randn(classes, D, generator=g), 0.1 * torch.randn(classes, generator=g)
    return x, gamma, beta, W, hb


def head_bwd_inputs(B, classes, D, dt):
    g = _gen(3 * B + classes + D)
    dl = torch.randn(B, classes, generator=g) / B
    xn = torch.randn(B, D, generator=g).to(dt)
    W = 0.02 * torch.randn(classes, D, generator=g)
    return dl, xn, W


def xent_inputs(B, C):
    """row b of: spread up to +-80; the maximum repeated; all logits equal; labels on the maximum (even b) / the minimum (odd b)"""
    g = _gen(11 * B + C)
    l = torch.randn(B, C, generator=g) * 3
    l[0] = (torch.rand(C, generator=g) * 160 - 80)
    if B > 1:
        l[1, : max(C // 2, 1)] = l[1].max()
    if B > 2:
        l[2] = 1.5
    y = torch.where(torch.arange(B) % 2 == 0, l.argmax(1), l.argmin(1))
    return l, y


def adamw_inputs(n, step, seed=0):
    """parameters of 1e-4, 1 and 1e3, gradients of exactly 0 (v -> 0: eps dominates), 1e-8, 1e4 and O(1) in one tensor; moments of
    a run that has lasted `step` steps"""
    g = _gen(seed + n + step)
    i = torch.arange(n)
    p = torch.randn(n, generator=g) * torch.tensor([1e-4, 1.0, 1e3])[i % 3]
    gr = torch.randn(n, generator=g) * torch.tensor([0.0, 1e-8, 1e4, 1.0])[(i // 3) % 4]
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m = 0.1 * torch.randn(n, generator=g) * torch.tensor([0.0, 1e-8, 1e4, 1.0])[(i // 3) % 4]
        v = m * m * (1 + torch.rand(n, generator=g))
    return p, gr, m, v


def share(mask):
    return float(mask.double().mean()) if mask.numel() else 0.0


def _cap(caps, dt, family):
    """a cap is a number, or {row family: number or None}"""
    return caps[family] if isinstance(caps, dict) else caps


def check_16(name, dev, vd, dt, caps, frac=1.0, fam=None):
    """the 16-bit rule of oracle.small_kernels.hold_16; the share of neighbour cases is taken per row family (fam: family of each
    row) where the cap depends on it"""
    ok, nb, ratio = K.hold_16(dev, vd[0], vd[1], dt)
    groups = {None: nb} if fam is None else {f: nb[[i for i, g in enumerate(fam) if g == f]] for f in sorted(set(fam))}
    used = {f: share(m) for f, m in groups.items()}
    print(f"  {name}: worst/bound {ratio:.3f}  neighbours " +
          " ".join(f"{'' if f is None else FAMILIES[f] + ' '}{s:.4f}/{_cap(caps, dt, f)}" for f, s in used.items()))
    assert ok.all(), f"{name}: {int((~ok).sum())}/{ok.numel()} outside the derived bound (worst ratio {ratio:.3f})"
    for f, s in used.items():
        cap = _cap(caps, dt, f)
        if cap is None:   # (a family whose derived term exceeds a 16-bit step: the interval alone holds it, see tolerances.py)
            continue
        assert s <= cap * frac, f"{name} {'' if f is None else FAMILIES[f]}: {s:.4f} neighbour cases, more than {frac:g} x cap {cap:g}"
    return ratio, used


def check_32(name, dev, vd):
    ok, ratio = K.hold_f32(dev, vd[0], vd[1])
    print(f"  {name}: worst/bound {ratio:.3f}")
    assert ok.all(), f"{name}: {int((~ok).sum())}/{ok.numel()} outside the derived bound (worst ratio {ratio:.3f})"
    return ratio


def fails_16(dev, vd, dt, caps, fam=None):
    try:
        check_16("slip", dev, vd, dt, caps, 1.0, fam)
    except AssertionError:
        return True
    return False


def fails_32(dev, vd):
    return not K.hold_f32(dev, vd[0], vd[1])[0].all()


DTYPES = [torch.bfloat16, torch.float16]


XU_RANKS = [(16, 32), (32, 32), (64, 64)]


def xu_factor(Rp, C, rank, dt, seed=6):
    """the packed factor Ut [Rp, C] of the fused contraction: rows beyond the rank are zero"""
    u = (0.1 * torch.randn(Rp, C, generator=_gen(seed))).to(dt)
    u[rank:] = 0
    return u


def xu_f32(y16, Ut, dt, slip=None):
    """fp32 T = y U in another order: 64 lanes own contiguous runs of K and add them last to first, adjacent lanes pair up"""
    y, u = y16.float(), Ut.float()
    if slip == "last_panel":   # the last 32-column K step left out
        y = y.clone()
        y[:, -32:] = 0
    return tree_sum(y[:, None, :] * u[None, :, :]).to(dt)


class Shares:
    """neighbour cases of one output summed over the cases of a test (the M of one C, rank and build): a tensor of M = 1 has 32
    elements, where one neighbour case is already 3 %"""

    def __init__(self):
        self.n, self.total = 0, 0

    def add(self, dev, vd, dt):
        ok, nb, ratio = K.hold_16(dev, vd[0], vd[1], dt)
        self.n, self.total = self.n + int(nb.sum()), self.total + nb.numel()
        return ok, ratio

    @property
    def share(self):
        return self.n / max(self.total, 1)
