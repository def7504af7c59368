"""Cases, operand families, the fp32 other-order restatements with their slips and the check helpers shared by
tests/test_skinny_model.py (host) and tests/test_skinny_contract_gpu.py (device).  The float64 restatement and its derived terms:
oracle/skinny_model.py; the caps on neighbour cases: tests/tolerances.py (SKINNY_CAPS)."""
import math

import torch

from oracle import gemm_model as G
from oracle import skinny_model as K
from tests import tolerances as T
from tests.gemm_common import DTYPES, check_16, check_32, dot_f32, lanes_for, rider_rows   # noqa: F401
from tests.small_kernels_common import tree_sum

# --- cara_skinny_xu(_r) ---------------------------------------------------------------------------------------------------------
XU_M = [1, 17, 63, 64, 65, 509, 512, 513]
XU_K = [32, 192, 224, 768, 3072, 3264]
XU_RANKS = [(32, 32), (32, 16), (32, 3), (64, 64), (64, 33), (64, 16)]


def xu_branches(M, Kc, Rp, rank):
    """Every decision of the launch and of its kernel that this (M, K, Rp, rank) takes, as a set of (decision, side) pairs: the pair (M, K)
    itself (the kernel choice, the wave count and the row-group count hang on both), the template and grid with the rank's class, and the
    store tails with the template"""
    p = K.xu_plan(M, Kc, Rp, rank)
    tmpl = (p["kernel"], p["groups"], p["NT"], p["grid_y"])
    return {("M, K", M, Kc), ("template, grid, rank class", tmpl, Rp, rank == Rp, rank <= 16), ("tails", tmpl, M % 4 != 0, M % 16 != 0, M < 16),
            ("waves", tmpl, p["waves"], (Kc // 32) % 4 != 0)}


def _prune():
    """The pruning rule: walk the product M x K x (Rp, rank) in the order of the three lists above (the rank list rotated by the position
    of (M, K), so that the first pick varies) and keep a triple iff it takes at least one (decision, side) pair of xu_branches that no
    triple kept before it takes.  Every pair that the full product reaches is therefore reached by a kept case -- every (M, K) at least
    once -- and a triple that differs from the kept ones in no branch is dropped."""
    seen, kept = set(), []
    for i, M in enumerate(XU_M):
        for j, Kc in enumerate(XU_K):
            for n in range(len(XU_RANKS)):
                Rp, rank = XU_RANKS[(n + i + j) % len(XU_RANKS)]
                b = xu_branches(M, Kc, Rp, rank)
                if not b <= seen:
                    seen |= b
                    kept.append((M, Kc, Rp, rank))
    return kept


XU_CASES = _prune()
# (M, K, Rp, rank, layout): ldx = K + 8 and panel-major X (ldx = -M, and -ldx > M) through both kernels
XU_LAYOUTS = [(65, 768, 32, 32, "ldx+8"), (65, 224, 32, 32, "ldx+8"), (513, 768, 64, 33, "panels"), (65, 768, 32, 16, "panels+"), (17, 224, 64, 64, "panels"),
              (65, 3264, 32, 32, "panels+")]
# (M, ldt): the buffer shared (ldt > roundup32(M): the pad is zeroed, the columns behind it are left); the pad does not fit (ldt = M = 40)
XU_LDT = [(65, 128), (17, 64), (40, 40)]

# --- cara_tskinny_* -------------------------------------------------------------------------------------------------------------
TS_M = [1, 32, 33, 128, 129, 257, 385, 513, 1000]
TS_K1 = [64, 128, 768]
TS_RANKS = [(32, 32), (32, 16), (32, 5), (64, 64), (64, 40)]
# Found while pinning ts_chunks: a chunk holds at most 8 steps until ceil(256 / colblocks) caps the chunk count, so the lists above reach
# waves of 0, 1 and 2 steps only.  (2000, 3264): 51 column blocks -> 6 chunks of 10 or 11 steps: waves of 3 steps, the third wait path of
# the ring.  Waves of >= 4 steps need M >= 2305 at K1 <= 3264; tests/test_kernels_gpu.py::test_tskinny (M = 12608: 5 steps) holds them
# to the same derived bound.  (Rp, rank) there: the one-r-tile form and the two-pass combine.
TS_EXTRA = [(2000, 3264)]
TS_EXTRA_RANKS = [(32, 16), (64, 64)]
TS_MK = [(M, K1) for M in TS_M for K1 in TS_K1] + TS_EXTRA


def ts_ranks(M, K1):
    return TS_EXTRA_RANKS if (M, K1) in TS_EXTRA else TS_RANKS


TN_MN = [(128, 128), (256, 128), (128, 384)]
TN_K = [1, 31, 32, 33, 64, 95, 333]
TN_NSLAB = [1, 2, 3]
TN_CASES = [(M, N, Kc, ns) for (M, N) in TN_MN for Kc in TN_K for ns in TN_NSLAB if K.tn_kslab(Kc, ns) is not None]
# (in, out, rank, Rp) x M
LIN_GEOMS = [(192, 256, 5, 32), (256, 192, 40, 64)]
LIN_M = [33, 200]


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * p for k, p in zip(key, (1, 7919, 104729, 1299709, 15485863))) % (2 ** 31))


def xu_operands(M, Kc, Rp, rank, dt, seed=0):
    """X [M, K]: row i of family (M - 1 - i) % 5 (the last row Gaussian, so M = 1 is) -- Gaussian; all zero; one outlier of 300 among
    O(1); tiny (1e-4); cancelling (+-1 alternating along K against the rows r % 8 == 1 of Ut, positive and nearly constant: |sum| << sum
    |.|).  Ut [Rp, K] Gaussian of scale 0.4 / sqrt(K), rows r % 8 == 2 and the rows at and above the rank zero."""
    g = _gen(seed, M, Kc, Rp, rank)
    fam = [(M - 1 - i) % 5 for i in range(M)]
    X = torch.randn(M, Kc, generator=g)
    for i, f in enumerate(fam):
        if f == 1:
            X[i] = 0.0
        elif f == 2:
            X[i, (17 * i + 5) % Kc] = 300.0
        elif f == 3:
            X[i] *= 1e-4
        elif f == 4:
            X[i] = (1.0 + 2.0 ** -6 * torch.randn(Kc, generator=g).round()) * (1.0 - 2.0 * (torch.arange(Kc) % 2))
    Ut = torch.randn(Rp, Kc, generator=g) * (0.4 / math.sqrt(Kc))
    r = torch.arange(Rp)
    Ut[r % 8 == 1] = 0.05 * (1.0 + 2.0 ** -6 * torch.randn(int((r % 8 == 1).sum()), Kc, generator=g).round())
    Ut[r % 8 == 2] = 0.0
    Ut[rank:] = 0.0
    return {"fam": fam, "X": X.to(dt), "Ut": Ut.to(dt)}


def ts_operands(M, K1, Rp, rank, dt, seed=0):
    """X = gemm_common.rider_rows (the five families by row; the cancelling rows cancel along M), Gt [Rp, roundup32(M)] zero but for
    [:rank, :M] Gaussian of scale 0.5"""
    g = _gen(seed, M, K1, Rp, rank, 1)
    X = rider_rows(M, K1, g)
    Gt = torch.zeros(Rp, K.roundup32(M))
    Gt[:rank, :M] = 0.5 * torch.randn(rank, M, generator=g)
    return {"X": X.to(dt), "Gt": Gt.to(dt)}


def tn_operands(M, N, Kc, dt, seed=0):
    """At [K, M] = rider_rows (the sums run over the rows: the cancelling family cancels along K), Bt [K, N] Gaussian of scale 0.4 with
    the columns n % 8 == 1 positive and nearly constant and n % 8 == 2 zero"""
    g = _gen(seed, M, N, Kc, 2)
    At = rider_rows(Kc, M, g)
    Bt = 0.4 * torch.randn(Kc, N, generator=g)
    n = torch.arange(N)
    Bt[:, n % 8 == 1] = 0.05 * (1.0 + 2.0 ** -6 * torch.randn(Kc, int((n % 8 == 1).sum()), generator=g).round())
    Bt[:, n % 8 == 2] = 0.0
    return {"At": At.to(dt), "Bt": Bt.to(dt)}


def lin_operands(geom, M, dt, seed=0):
    in_, out_, rank, Rp = geom
    g = _gen(seed, in_, out_, rank, M, 3)
    o = xu_operands(M, in_, Rp, rank, dt, seed)
    W = torch.randn(out_, in_, generator=g) * (0.4 / math.sqrt(in_))
    Vs = 0.3 * torch.randn(out_, Rp, generator=g)
    Vs[:, rank:] = 0
    o.update(W=W.to(dt), Vs=Vs.to(dt), bias=0.3 * torch.randn(out_, generator=g), aux=torch.randn(M, out_, generator=g),
             rowscale=torch.tensor([0.0, 1.0, 1.0 / 0.9])[(torch.arange((M + 16) // 17) + 1) % 3], rps=17,
             dY=(0.1 * rider_rows(M, out_, g)).to(dt))
    o["U"], o["Wt"], o["Vst"] = o["Ut"].t().contiguous(), o["W"].t().contiguous(), o["Vs"].t().contiguous()
    return o


# --- fp32 in another order, with the slips ---------------------------------------------------------------------------------------
SLIPS = {"a": "last K-slice / last wave's partial sum left out of T", "b": "row M - 1 of T from row M - 2 of X (clamp off by one)",
         "c": "column tiles 16 .. 31 left stale at rank <= 16", "d": "Tt's pad columns non-zero, consumed by xtg", "e": "column sums count the clamped rows",
         "f": "last 32-row step of a chunk dropped", "g": "a wave without steps adds a stale stage", "h": "the reduction drops its n % 4 tail",
         "i": "reduce_many at Rc = 16 reads slabs with stride Rp", "j": "tn's ragged step unmasked", "k": "tn's slab boundary shifted by 32 rows",
         "l": "T rounded to 16 bits before the sum over waves"}
XU_SLIPS, TS_SLIPS, TN_SLIPS = "abcl", "defghi", "jk"


def restate_xu(o, M, Kc, Rp, rank, dt, slip=None, lanes=32):
    """T in fp32: `lanes` lanes own contiguous runs of K (gemm_common.dot_f32; the kernels cut K into 192-wide slices or into steps w, w + 4,
    ...), rounded once -> {"T", "Tt"}"""
    p = K.xu_plan(M, Kc, Rp, rank)
    X, Ut = o["X"].float(), o["Ut"].float()
    if slip == "a":
        X = X.clone()
        if p["kernel"] == "sliced":
            X[:, Kc - 192:] = 0
        else:
            last = min(Kc // 32, 4) - 1
            X.view(M, Kc // 32, 32)[:, last::4] = 0
    if slip == "l":
        parts = ([slice(w * 192, w * 192 + 192) for w in range(Kc // 192)] if p["kernel"] == "sliced" else
                 [torch.arange(Kc).view(-1, 32)[w::4].reshape(-1) for w in range(min(Kc // 32, 4))])
        T32 = sum(dot_f32(X[:, s].contiguous(), Ut[:, s].contiguous(), 32).to(dt).float() for s in parts)
    else:
        T32 = dot_f32(X, Ut, lanes_for(Kc, lanes))
    Tm = T32.to(dt)
    if p["kernel"] == "sliced" and p["NT"] == 1:
        Tm[:, 16:] = 0.5 if slip == "c" else 0.0
    if slip == "b" and M >= 2:
        Tm[M - 1] = Tm[M - 2]
    return {"T": Tm, "Tt": Tm.t().contiguous()}


def xu_slip_applies(M, Kc, Rp, rank, slip):
    p = K.xu_plan(M, Kc, Rp, rank)
    return {"b": M >= 2, "c": p["kernel"] == "sliced" and p["NT"] == 1, "l": p["waves"] > 1}.get(slip, True)


def _pad_rows(X, M):
    Xp = torch.zeros(K.roundup32(M), X.shape[1])
    Xp[:M] = X[:M].float()
    return Xp


def restate_xtg(o, M, K1, Rp, rank, slip=None, lanes=32, half=False):
    """D = X^T G and the column sums in fp32 over the rows padded with zeros to a multiple of 32: `lanes` lanes own contiguous runs of
    rows, last to first, then pair up (the kernels cut the rows into chunks, then steps w, w + 4, ... of 32) -> {"D", "colsum"}"""
    Mp = K.roundup32(M)
    Xp, Gp = _pad_rows(o["X"], M), o["Gt"][:, :Mp].float().clone()
    Xc = Xp.clone()   # for the column sums
    chunks = K.ts_steps(M, K1)
    if slip == "d":      # the pad columns of Gt hold ones and the clamped rows of X (row M - 1) meet them
        Xp[M:] = Xp[M - 1]
        Gp[:rank, M:] = 1.0
    if slip == "e":
        Xc[M:] = Xc[M - 1]
    if slip == "f":
        b, e = chunks[0]
        Xp[(e - 1) * 32:e * 32] = 0
        Xc[(e - 1) * 32:e * 32] = 0
    if slip == "h":
        n = len(chunks)
        for b, e in chunks[n // 4 * 4:]:
            Xp[b * 32:e * 32] = 0
            Xc[b * 32:e * 32] = 0
    D = dot_f32(Xp.t().contiguous(), Gp, lanes)
    cs = tree_sum(Xc.t().contiguous(), lanes)
    if slip == "g":      # the stage a wave without steps never filled: the first step's tiles once more
        D = D + dot_f32(Xp[:32].t().contiguous(), Gp[:, :32].contiguous(), 32)
        cs = cs + tree_sum(Xc[:32].t().contiguous(), 32)
    if half:
        if slip == "i":  # slabs [chunk][colblock][64][16] read as if 32 wide
            parts = torch.stack([dot_f32(Xp[b * 32:e * 32].t().contiguous(), Gp[:16, b * 32:e * 32].contiguous(), 32) if e > b else torch.zeros(K1, 16) for b, e in chunks])
            flat = torch.cat((parts.reshape(-1), torch.zeros(parts.numel())))
            idx = (torch.arange(len(chunks))[:, None, None] * K1 * 32 + torch.arange(K1)[None, :, None] * 32 + torch.arange(16)[None, None, :])
            D = torch.cat((flat[idx].sum(0), torch.zeros(K1, 16)), 1)
        else:
            D[:, 16:] = 0.0
    return {"D": D, "colsum": cs}


def ts_slip_applies(M, K1, Rp, rank, slip, half=False):
    return {"d": M % 32 != 0, "e": M % 32 != 0, "g": 0 in K.ts_wave_steps(M, K1), "h": K.ts_chunks(M, K1) % 4 != 0, "i": half}.get(slip, True)


def restate_tn(o, M, N, Kc, nslab, slip=None, lanes=32):
    """every slab in fp32 over its rows padded with zeros to a multiple of 32 (`lanes` lanes own contiguous runs; the kernel walks them
    in steps of 32) -> [C_z]"""
    kslab = K.tn_kslab(Kc, nslab)
    out = []
    for z in range(nslab):
        lo, hi = z * kslab, min((z + 1) * kslab, Kc)
        if slip == "k":
            lo, hi = min(lo + 32, Kc), min(hi + 32, Kc)
        a, b = o["At"][lo:hi, :M].float(), o["Bt"][lo:hi, :N].float()
        rows = hi - lo
        ap, bp = torch.zeros(K.roundup32(max(rows, 1)), M), torch.zeros(K.roundup32(max(rows, 1)), N)
        ap[:rows], bp[:rows] = a, b
        if slip == "j" and rows % 32:
            ap[rows:], bp[rows:] = a[-1], b[-1]
        out.append(dot_f32(ap.t().contiguous(), bp.t().contiguous(), lanes))
    return out


def tn_slip_applies(M, N, Kc, nslab, slip):
    kslab = K.tn_kslab(Kc, nslab)
    return {"j": any((min((z + 1) * kslab, Kc) - z * kslab) % 32 for z in range(nslab)), "k": Kc > 32}.get(slip, True)


# --- the rules --------------------------------------------------------------------------------------------------------------------
def holds_xu(got, model, dt, quiet=True, name="T"):
    """T under the interval rule and the cap (SKINNY_CAPS), Tt bit for bit T transposed -> (ok, ratio, share)"""
    ok, ratio, used = check_16(name, got["T"], model["T"], dt, T.SKINNY_CAPS[name], quiet=quiet)
    if got.get("Tt") is not None:
        ok &= torch.equal(got["Tt"].contiguous().view(torch.int16), got["T"].t().contiguous().view(torch.int16))
    return ok, ratio, used


def holds_xtg(got, model, other, quiet=True, names=("D", "colsum")):
    """D and the column sums element by element and under check_32's aggregate rule -> {name: (ok, ratio, aggregate)}; columns the model
    states as exact zeros (d == 0) must be +0 in bits"""
    res = {}
    for n in names:
        if n not in model:
            continue
        v, d = model[n]
        exact = d == 0
        g = got[n].cpu()
        ok0 = bool((g[exact].contiguous().view(torch.int32) == 0).all()) if exact.any() else True
        keep = ~exact
        ok, ratio, agg = check_32(n, g[keep], (v[keep], d[keep]), None if other is None else other[n][keep], quiet=quiet)
        res[n] = (ok and ok0, ratio, agg)
    return res


def holds_tn(got, model, other, quiet=True):
    return {f"slab{z}": check_32(f"slab{z}", got[z], model[z], None if other is None else other[z], quiet=quiet) for z in range(len(model))}


def restate_lin_y(o, M, T_dev, lanes=32):
    """the CARA_EPI_RESID output of cara_linear_fwd in fp32, another order: aux + rs ([X | T] [W | Vs]^T + bias) with the device's T"""
    A = torch.cat((o["X"][:M].float(), T_dev.float()), 1)
    B = torch.cat((o["W"].float(), o["Vs"].float()), 1)
    u = dot_f32(A, B, lanes_for(A.shape[1], lanes)) + o["bias"]
    rs = o["rowscale"][torch.arange(M) // o["rps"]][:, None]
    return o["aux"] + rs * u
