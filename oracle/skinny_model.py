"""Plain float64 restatement of the skinny-product and dense-dW kernels as STAND-ALONE launches -- cara_skinny_xu(_r), cara_tskinny_partial*
with cara_tskinny_reduce(_many), cara_tskinny_xtg (cara_amd/csrc/skinny.hip, tskinny_body.h), cara_gemm_tn_f32 (gemm.hip) and the
compositions cara_linear_fwd / cara_linear_bwd (linear.hip) -- with a per-element term DERIVED from each kernel's arithmetic, in the
convention of oracle/gemm_model.py: every function returns (v, d) per output; a product of two 16-bit operands is exact in fp32, so
only the additions round; a 16x16x32 MFMA adds 32 products to its accumulator in an order the hardware does not state: at most 32
roundings; gamma, hold_f32 and hold_16 are used as they are.  Every count is read from the code (the lines are quoted in
docs/findings/skinny_contract.md); nothing is fitted.  The dispatch predicates of the entry points are restated here (xu_plan,
ts_chunks, tn_kslab) so that a test can say which kernel, with which template arguments, a shape runs.
tests/test_skinny_model.py proves on the host that an fp32 restatement in another order stays inside every bound and that twelve
plausible slips do not; tests/test_skinny_contract_gpu.py then holds the device to it."""
import torch

from oracle import gemm_model as G
from oracle.gemm_model import TINY, gamma, f64, kappa_red

XU_KSLICE, XU_GROUPS, TS_COLS, TS_TARGET_BLOCKS, TS_REDUCE_MAX = 192, 4, 64, 256, 24   # (CARA_TS_REDUCE_MAX: include/cara_hip.h)


def roundup32(M):
    return (M + 31) // 32 * 32


# ----------------------------------------------------------------------------------------------------------------------------
# T = X Ut^T  (cara_skinny_xu_r)
# ----------------------------------------------------------------------------------------------------------------------------
def xu_plan(M, K, Rp, rank):
    """The launch cara_skinny_xu_r chooses (the predicate of the C code, skinny.hip: `if ((Rp == 32 || Rp == 64) && K % XU_KSLICE == 0 &&
    K / XU_KSLICE <= 16 && M >= 64)`) -> dict(kernel, NT, groups, grid_y, waves, kappa).

    sliced (skinny_xu_sliced_kernel): wave w owns K-slice [192 w, 192 w + 192): KS = 6 MFMA steps on one accumulator (`for (int ks = 0;
        ks < KS; ++ks) ... acc[j] = mfma(a[ks], u[ks][j], acc[j])`: 6 x 32 = 192 roundings), then `s[.] += v[.]` over the other
        nwaves - 1 = K / 192 - 1 waves in sequence:  kappa = 192 + (K / 192 - 1).
    v1 (skinny_xu_kernel): wave w takes the k-steps w, w + 4, ... of K / 32: ceil(K / 32 / 4) MFMAs, then `s[.] += v[.]` over w = 1 .. 3
        (3, whether those waves had a step or left zeros):  kappa = 32 ceil(K / 32 / 4) + 3.
    groups: `M <= 16 * XU_GROUPS * 8 ? 1 : XU_GROUPS`;  NT = 1 iff Rp == 32 && rank <= 16 (sliced only; grid.y = 1);  otherwise the
    sliced kernel runs NT = 2 with grid.y = Rp / 32, and v1 NT = Rp / 16."""
    nks = K // 32
    if Rp in (32, 64) and K % XU_KSLICE == 0 and K // XU_KSLICE <= 16 and M >= 64:
        nw = K // XU_KSLICE
        nt1 = Rp == 32 and rank <= 16
        return dict(kernel="sliced", NT=1 if nt1 else 2, groups=1 if M <= 16 * XU_GROUPS * 8 else XU_GROUPS, grid_y=1 if nt1 else Rp // 32,
                    waves=nw, kappa=192 + (nw - 1))
    return dict(kernel="v1", NT=Rp // 16, groups=1, grid_y=1, waves=min(nks, 4), kappa=32 * -(-nks // 4) + 3)


def xu(X, Ut, M, K, Rp, rank, ldt=None):
    """X [>= M, K], Ut [Rp, K] 16-bit -> {"T": (v, d) [M, Rp], "Tt": (v^T, d^T), "pad": (M, hi), "plan": xu_plan}.
    d = gamma(kappa) |X||Ut|^T.  Under NT = 1 the columns 16 .. 31 are exact zeros whatever Ut holds (`T[...] = (bf16)0.f`); columns
    whose rows of Ut are zero come out as exact zeros in every kernel (sums of exact zero products).  Tt is T transposed bit for
    bit (the same `(bf16)s[r]` values); its columns [M, min(roundup32(M), ldt)) are zero when roundup32(M) <= ldt (the
    hipMemset2DAsync of the entry point, skipped otherwise): "pad" is that column range (empty when skipped); nothing at or beyond ldt,
    or between the pad and ldt, is written."""
    plan = xu_plan(M, K, Rp, rank)
    Xd, Ud = f64(X)[:M, :K], f64(Ut)[:, :K]
    v = Xd @ Ud.t()
    d = gamma(plan["kappa"]) * (Xd.abs() @ Ud.abs().t()) + TINY
    if plan["kernel"] == "sliced" and plan["NT"] == 1:
        v[:, 16:] = 0.0
        d[:, 16:] = 0.0
    m32 = roundup32(M)
    hi = m32 if (ldt is not None and m32 <= ldt) else M
    return {"T": (v, d), "Tt": (v.t(), d.t()), "pad": (M, hi), "plan": plan}


# ----------------------------------------------------------------------------------------------------------------------------
# D = X^T G, colsum = sum_m X  (cara_tskinny_partial* + cara_tskinny_reduce*)
# ----------------------------------------------------------------------------------------------------------------------------
def ts_chunks(M, K1):
    """ts_chunks of tskinny_body.h, line by line"""
    colblocks = K1 // TS_COLS
    c = (TS_TARGET_BLOCKS + colblocks - 1) // colblocks
    steps = (M + 31) // 32
    maxc = (steps + 7) // 8
    return max(min(c, maxc), 1)


def ts_scratch_bytes(M, K1, Rp):
    """cara_tskinny_scratch_bytes with helper waves off: one slab [64, Rp] fp32 and 64 column sums per block"""
    blocks = (K1 // TS_COLS) * ts_chunks(M, K1)
    return blocks * TS_COLS * Rp * 4 + blocks * TS_COLS * 4


def ts_steps(M, K1):
    """-> [(s_begin, s_end)] per chunk: `s_begin = steps * chunk / nchunks, s_end = steps * (chunk + 1) / nchunks` (tskinny_body)"""
    steps, n = (M + 31) // 32, ts_chunks(M, K1)
    return [(steps * c // n, steps * (c + 1) // n) for c in range(n)]


def ts_wave_steps(M, K1):
    """the set of nmine = steps of one wave over all (chunk, wave): which wait paths of the 3-stage ring a shape exercises"""
    out = set()
    for b, e in ts_steps(M, K1):
        for w in range(4):
            out.add((e - (b + w) + 3) // 4 if b + w < e else 0)
    return out


def kappa_xtg(M, K1):
    """(kappa_D, kappa_cs) of the stand-alone launch for the nchunks ts_chunks returns: the count of gemm_model.kappa_ts_form("tskinny")
    at THAT nchunks instead of its maximum over all of them.  A chunk holds at most ceil(steps / nchunks) steps, a wave nm = ceil(that / 4)
    MFMAs on one accumulator (32 nm); `s[.] += v[.]` adds the other three waves (3); the reduction (strided_sum4 / strided_sum4_v) runs
    over nchunks slabs: kappa_red(nchunks).  Column sums: `csum[it] += (float)b[j]` eight times a step (8 nm), `s += cred[...]` over 4 waves x
    4 row groups from 0.f (16), the same reduction."""
    nm = -(-max(e - b for b, e in ts_steps(M, K1)) // 4)
    red = kappa_red(ts_chunks(M, K1))
    return 32 * nm + 3 + red, 8 * nm + 16 + red


def xtg(X, Gt, M, K1, Rp, rank, colsum=True, half=False):
    """X [>= M, K1] 16-bit, Gt [Rp, >= roundup32(M)] 16-bit whose columns [M, roundup32(M)) are ZERO (the caller's contract: the rows of X
    behind M - 1 are clamped to row M - 1, not masked) -> {"D": (v, d) [K1, Rp], "colsum": (v, d) [K1]} after the reduction.
    half: the one-r-tile form (cara_tskinny_partial2_r at Rp = 32, rank <= 16, reduced with Rc = 16): columns 16 .. 31 of D are exact zeros
    (`r < Rc ? ... : f32x4{0.f, ...}`).  Columns whose rows of Gt are zero are exact zeros in every form."""
    kd, kc = kappa_xtg(M, K1)
    o = G.rider_products(f64(X)[:, :K1], Gt, M, (kd, kc))
    v, d = o["D"]
    if half:
        v[:, 16:] = 0.0
        d[:, 16:] = 0.0
    out = {"D": (v, d)}
    if colsum:
        out["colsum"] = o["colsum"]
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# C[z] = At[rows of slab z]^T Bt[rows of slab z]  (cara_gemm_tn_f32)
# ----------------------------------------------------------------------------------------------------------------------------
def tn_kslab(K, nslab):
    """`kslab = ((K + nslab - 1) / nslab + 31) / 32 * 32` -> kslab, or None where the entry refuses the pair (`kslab * (nslab - 1) >= K`:
    an empty last slab)"""
    if nslab <= 0 or nslab > 65535:
        return None
    kslab = ((K + nslab - 1) // nslab + 31) // 32 * 32
    return None if kslab * (nslab - 1) >= K else kslab


def tn(At, Bt, M, N, K, nslab):
    """At [K, >= M], Bt [K, >= N] 16-bit -> [(v, d)] per slab z over ITS rows [z kslab, min((z + 1) kslab, K)) only: gemm_tn_kernel runs
    nk = ceil(rows / 32) steps `acc[i][j] = mfma(a[i], b[j], acc[i][j])` on one accumulator (the last one ragged: rows clamped to
    k_end - 1 and the A fragments of rows >= k_end set to zero -- exact zero products), the epilogue stores the fp32 accumulator:
    kappa = 32 ceil(rows / 32)."""
    kslab = tn_kslab(K, nslab)
    assert kslab is not None
    A, B = f64(At)[:K, :M], f64(Bt)[:K, :N]
    out = []
    for z in range(nslab):
        a, b = A[z * kslab:min((z + 1) * kslab, K)], B[z * kslab:min((z + 1) * kslab, K)]
        out.append((a.t() @ b, gamma(32 * -(-a.shape[0] // 32)) * (a.abs().t() @ b.abs()) + TINY))
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# cara_linear_fwd / cara_linear_bwd (linear.hip): compositions of the above and of cara_gemm_bf16
# ----------------------------------------------------------------------------------------------------------------------------
def linear_fwd(X, W, bias, Ut, Vs, M, Rp, rank, epi, dt, T_dev, ldt=None, aux=None, rowscale=None, rows_per_sample=1):
    """`cara_skinny_xu_r(X, ldx, L->Ut, T, Tt, ldt, M, L->in, L->Rp, L->rank)` then `cara_gemm_bf16` of [X | T] [W | Vs]^T + bias with the
    epilogue: T / Tt from xu(); Y from gemm_model.accumulate with the T the DEVICE wrote as the extension's operand (its convention:
    T's own rounding ties stay out of Y's bound) and gemm_model.epilogue."""
    K = W.shape[1]
    o = xu(X, Ut, M, K, Rp, rank, ldt)
    acc = G.accumulate(f64(X)[:M, :K], W, T_dev, Vs)
    o["Y"] = G.epilogue(epi, acc, dt, bias=bias, aux=aux, rowscale=rowscale, rows_per_sample=rows_per_sample)["C"]
    return o


def linear_bwd(dY, X, Wt, U, Vst, M, Rp, rank, dt, G_dev, Gt_dev, Tt_dev, ldt=None):
    """G' = dY Vs (xu), dX = [dY | G'] [W^T | U]^T (CARA_EPI_BF16, no bias; the device's G' as operand), dU = X^T G' and dVs = dY^T T with
    dc = colsum dY (cara_tskinny_partial2_r + cara_tskinny_reduce_many, Rc = 16 at Rp = 32 and rank <= 16; the device's Gt and Tt as
    operands)."""
    out_, in_ = Wt.shape[1], Wt.shape[0]
    g = xu(dY, Vst, M, out_, Rp, rank, ldt)
    half = Rp == 32 and rank <= 16
    o = {"G": g["T"], "Gt": g["Tt"], "pad": g["pad"], "plan": g["plan"]}
    o["dX"] = G.epilogue(G.EPI_BF16, G.accumulate(f64(dY)[:M, :out_], Wt, G_dev, U), dt)["C"]
    o["dU"] = xtg(X, Gt_dev, M, in_, Rp, rank, colsum=False, half=half)["D"]
    v = xtg(dY, Tt_dev, M, out_, Rp, rank, colsum=True, half=half)
    o["dVs"], o["dc"] = v["D"], v["colsum"]
    return o
