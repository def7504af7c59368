"""Plain float64 restatement of the GEMM family -- cara_gemm_bf16 / cara_gemm_with_tskinny_r of cara_amd/csrc/gemm.hip, gemm8.hip,
gemm_epilogue.h and the products that ride in their launches -- with a per-element term DERIVED from each kernel's arithmetic, in
the convention of oracle/small_kernels.py (whose U, gamma, f64, round16, hold_f32 and hold_16 are used as they are).

Every function returns (v, d) per output: v the float64 value with a 16-bit rounding exactly where the kernel rounds, d how far the
kernel's fp32 value may lie from v.  A product of two 16-bit operands is exact in fp32 (bf16: 16 significand bits, fp16: 22), so
in the accumulator only the ADDITIONS round; `acc = mfma_f32_16x16x32(a, b, acc)` adds 32 products to the accumulator in an order
the hardware does not state: at most 32 roundings per step (the convention of small_kernels.kappa_xu).  Nothing here is fitted to a
device: tests/test_gemm_model.py proves on the host that an fp32 restatement in another order stays inside every bound and that
twelve plausible slips do not; tests/test_gemm_contract_gpu.py then holds the device to it.
"""
import math

import torch

from oracle.small_kernels import U, gamma, f64, round16, hold_f32, hold_16   # noqa: F401  (re-exported: the two rules)

TINY = 2.0 ** -149
FAM_TILE8, FAM_TILE8_256, FAM_FT, FAM_G32, FAM_BATCHED, FAM_FEW_ROWS = 1, 2, 3, 4, 5, 6
EPI_BF16, EPI_F32, EPI_GELU, EPI_RESID, EPI_DGELU, EPI_GELU_DG, EPI_MULH = range(7)


def kappa_gemm(family, K, Rp=0, twob=False, block=256):
    """Roundings on the longest path into one accumulator element, per kernel family.

    FAM_G32 / FAM_BATCHED (gemm32_body, gemm.hip): ONE chain `mma_tile32(sA, sA + A_BYTES, acc, ...)` over ntot = K / 32 + Rp / 32
        steps (`for (int kt = 0; kt < ntot; ++kt)`: the K-extension is the tail of the same loop); with B3 (mma_tile32_2b) every
        step runs two MFMAs on the same accumulator, 2 K / 32 steps, and the extension follows (`for (int kk = 0; kk < (p.Rp >> 5)`).
        32 roundings per step:  kappa = 32 (K / 32 (1 + twob) + Rp / 32) = K (1 + twob) + Rp.  The 128- and the 160-row tile differ in
        MI (rows per wave) only.
    FAM_FT (gemm32ft_body): the same chain over K / 32 steps, then `mma_tile32<4>(sE, ...)` and, NU = 2, `mma_tile32<4>(sO, ...)`:
        K + Rp as above (Rp = 32: columns 16 .. 31 of the 16-column form are zeros that are still added).
    FAM_TILE8 / FAM_TILE8_256 (gemm8.hip): a K step of 64 is four phases, each an MFMA cluster of one quadrant of the wave's
        outputs; an accumulator element sees two 16x16x32 MFMAs per K step, in the order of K, and one more for the extension --
        the file's header and tests/test_gemm8_gpu.py (bit for bit the 128-row kernel) say the same chain: K + Rp.  Helper waves
        (mode 3) compute T, not C; DV reads the A sub-buffers and adds nothing to acc: neither changes the count.
    FAM_FEW_ROWS (small_m_direct_kernel): NW = block / 64 waves split the K / 32 steps (wave w: steps w, w + NW, ...), each a chain
        of ceil(K / 32 / NW) MFMAs; `t += red[w][...]` adds the NW partial tiles in sequence (NW: t starts at 0); small_m_finish4
        then adds the adapter term d (a chain of Rp `d += a b`: Rp roundings, a contracted fma only removes some) with one more:
        kappa = 32 ceil(K / 32 / NW) + NW + (Rp + 1 if Rp).
    The T of the adapter inside (kappa_T): `accg = mfma(a, bu, accg)` over the K / 32 steps: K."""
    if family == FAM_FEW_ROWS:
        nw = block // 64
        return 32 * -(-(K // 32) // nw) + nw + ((Rp + 1) if Rp else 0)
    return K * (2 if twob else 1) + Rp


def kappa_T(K):
    return K


def accumulate(A, B, A2=None, B2=None, B3=None, *, family=FAM_G32, block=256):
    """acc = A B^T [+ A2 B2^T] [+ A B3^T] -> (v, d), d_acc = gamma(kappa_gemm) (|A||B|^T + |A2||B2|^T + |A||B3|^T).  A2 is the 16-bit
    T the extension reads: given by the caller, or -- the adapter inside -- the T_out the device wrote (the convention of the older
    tests: T's own rounding ties stay out of C's bound; T is held by adapter_T)."""
    A, B = f64(A), f64(B)
    v, s = A @ B.t(), A.abs() @ B.abs().t()
    Rp = 0
    if A2 is not None:
        A2, B2 = f64(A2), f64(B2)
        Rp = A2.shape[1]
        v, s = v + A2 @ B2.t(), s + A2.abs() @ B2.abs().t()
    if B3 is not None:
        B3 = f64(B3)
        v, s = v + A @ B3.t(), s + A.abs() @ B3.abs().t()
    k = kappa_gemm(family, A.shape[1], Rp, B3 is not None, block)
    return v, gamma(k) * s + TINY


def adapter_T(A, Ut, rank=None):
    """T = (16-bit)(A Ut^T) of the adapter inside (gemm32ft_body: `accg[i][c] = mfma(a[i], bu[c], accg[i][c])`, rounded by `bf16x4 tv =
    {(bf16)av[0], ...}`; gemm8.hip modes 2 / 3 the same sum): d_T = gamma(kappa_T(K)) |A||Ut|^T.  Columns beyond the rank (zero rows
    of Ut; at Ut_rank <= 16 columns 16 .. 31 are not computed but written as zeros) are exact zeros: d = 0 there but for the
    denormal."""
    A, Ut = f64(A), f64(Ut)
    return A @ Ut.t(), gamma(kappa_T(A.shape[1])) * (A.abs() @ Ut.abs().t()) + TINY


# ----------------------------------------------------------------------------------------------------------------------------
# gelu_erf / gelu_erf_grad of common.h, as written
# ----------------------------------------------------------------------------------------------------------------------------
def _c32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def _mul32(a, b):
    return float(torch.tensor(a, dtype=torch.float32) * torch.tensor(b, dtype=torch.float32))


C1 = _mul32(0.3275911, 0.70710678118654752)          # `0.3275911f * 0.70710678118654752f`: one fp32 constant
C2 = _mul32(-0.5, 1.4426950408889634)                # `-0.5f * 1.4426950408889634f`
C3 = _c32(0.39894228040143268)
POLY = [0.5 * _c32(c) for c in (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)]   # (the halving is exact)


def _half_poly(au, usq):
    """gelu_half_poly (common.h) in float64 with its fp32 constants: t = 1 / (1 + C1 |u|), e = exp2(u^2 C2), hp = P(t) / 2.
    -> t, e, hp, S = sum |c_i| t^i (what the Horner roundings scale with), d_hp, d_e: the fp32 evaluation's distances.

    t: the fma one rounding (u), v_rcp_f32 1 ulp = 2u: 3u t.  hp: five Horner levels `t * (c + ...)`, at most two roundings each
    (10u S), and t's error moves a polynomial of degree 5 by at most 5 * 3u S:  d_hp = 25u S.
    e: u u one rounding, the product with C2 another: the exponent x = u^2 C2 is off by 2u |x|, which moves exp2 by 2u |x| ln 2
    relative; v_exp_f32 1 ulp = 2u; results below 2^-126 are flushed:  d_e = e (2 |x| ln 2 + 2) u + 2^-126."""
    t = 1.0 / (1.0 + C1 * au)
    x = usq * C2
    e = torch.exp2(x)
    hp, S = torch.zeros_like(t), torch.zeros_like(t)
    for c in reversed(POLY):
        hp, S = t * (c + hp), t * (abs(c) + S)
    return t, e, hp, S, 25 * U * S, e * (2 * x.abs() * math.log(2) + 2) * U + 2.0 ** -126


def gelu(u, d_u=None):
    """gelu_erf (common.h): `fmaf(-(au * hp), e, fmaxf(u, 0.f))` -> (v, d).  au hp one rounding, the fma one:
        d = |u| e d_hp + |u| hp d_e + u |u| hp e + u |g|   (+ 1.13 d_u: |gelu'| <= 1.13, for an argument known to d_u)."""
    u = f64(u)
    au = u.abs()
    t, e, hp, S, d_hp, d_e = _half_poly(au, u * u)
    g = u.clamp_min(0.0) - au * hp * e
    d = au * e * d_hp + au * hp * d_e + U * au * hp * e + U * g.abs() + TINY
    return g, d + (1.13 * d_u if d_u is not None else 0.0)


def gelu_grad(u, d_u=None):
    """gelu_erf_grad: half_erf = fma(-hp, e, 0.5) (e d_hp + hp d_e + u / 2), cdf = 0.5 + copysign(half_erf, u) (u), the result
    fma(u C3, e, cdf): u C3 one rounding, d_e through |u| C3, the fma one:
        d = e d_hp + hp d_e + 1.5u + |u| C3 (u e + d_e) + u |g'|   (+ 0.8 d_u: |gelu''| = |phi(u) (2 - u^2)| <= 2 phi(0) = 0.798)."""
    u = f64(u)
    au = u.abs()
    t, e, hp, S, d_hp, d_e = _half_poly(au, u * u)
    half_erf = 0.5 - hp * e
    cdf = 0.5 + torch.copysign(half_erf, u)
    gp = u * C3 * e + cdf
    d = e * d_hp + hp * d_e + 1.5 * U + au * C3 * (U * e + d_e) + U * gp.abs() + TINY
    return gp, d + (0.8 * d_u if d_u is not None else 0.0)


ERF_ABS = 1.5e-7 + 14 * U
"""Distance of the RESTATEMENT's erf from the true erf: Abramowitz-Stegun 7.1.26 is good to 1.5e-7 ABSOLUTE with its exact
constants; the kernel's constants are those rounded to fp32 (u relative each): C1 moves t by u t, i.e. P(t) / 2 by at most 5u S, the
coefficients by u S, C2 moves e by u |x| ln 2 e (<= 0.6u): erf = 1 - 2 (P / 2) e moves by at most 2 (6 S + 0.6) u <= 14u (S <= 1.12)."""


def gelu_vs_true(u):
    """-> (true erf GELU, true derivative, bound on |restatement - true| for gelu, for gelu') in float64.
    gelu = u (1 + erf(u / sqrt 2)) / 2: the erf error carried through |u| / 2.  The term is ABSOLUTE: on the negative tail --
    gelu(-5) = -1.4e-6 against a term of 2.4e-6 -- it, not a relative bar, is what holds the output; the kernel's gelu there is
    the difference max(u, 0) - |u| (P / 2) e of two nearly equal numbers and carries no correct digit of the true value.
    gelu' = Phi(u) + u phi(u): Phi carries ERF_ABS / 2, and u phi(u) = u C3 e the fp32 constants' 2u (1 + |x| ln 2) relative."""
    u = f64(u)
    true = 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))
    phi = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    true_g = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * phi
    x = (u * u * C2).abs()
    return true, true_g, u.abs() / 2 * ERF_ABS + TINY, ERF_ABS / 2 + (u * phi).abs() * 2 * U * (1 + x * math.log(2)) + TINY


# ----------------------------------------------------------------------------------------------------------------------------
# the seven epilogues (gemm_epilogue.h: epilogue_rows and its fast forms; small_m_finish4 of gemm.hip)
# ----------------------------------------------------------------------------------------------------------------------------
def epilogue(epi, acc, dt, *, bias=None, aux=None, rowscale=None, rows_per_sample=1, want_c2=True):
    """acc = (v, d) of accumulate() -> {"C": (v, d)[, "C2": (v, d)]}; a 16-bit output's v is the float64 value BEFORE its final
    rounding (hold_16 rounds).  Every form of every epilogue does the same operations in the same association:
      bias:  `v = a + bv` one rounding (u |u|) where a bias is given (a NULL bias adds 0.f: exact).
      CARA_EPI_BF16 / _F32:  C = acc + bias.
      CARA_EPI_GELU:  C2 = (16-bit) u, C = (16-bit) gelu_erf(u) of the UNROUNDED fp32 u (`out2[k] = (bf16)v[k]; out[k] =
          (bf16)gelu_erf(v[k])`): d_C = gelu's own term + 1.13 d_u.
      CARA_EPI_GELU_DG:  the same C, C2 = (fp16, whatever the build) gelu_erf_grad(u) (`outh[k] = (h16)gp`).
      CARA_EPI_RESID:  C = aux + rs (acc + bias), in exactly that association (`x[k] + rs * v[k]`): the product and the sum one
          rounding each (a contracted fma removes one): d = |rs| d_u + u |rs u| + u |C|.
      CARA_EPI_DGELU:  C = (16-bit)(u gelu_erf_grad((float)aux16)): aux is the 16-bit pre-activation, an exact input:
          d = |g'| d_u + |u| d_g' + u |C|.
      CARA_EPI_MULH:  C = (16-bit)(acc * (float)aux_fp16) (no bias): d = |aux| d_acc + u |C|."""
    v, d = acc
    M = v.shape[0]
    if bias is not None:
        v = v + f64(bias)
        d = d + U * v.abs()
    if epi in (EPI_BF16, EPI_F32):
        return {"C": (v, d)}
    if epi in (EPI_GELU, EPI_GELU_DG):
        out = {"C": gelu(v, d)}
        if want_c2:
            out["C2"] = (v, d) if epi == EPI_GELU else gelu_grad(v, d)
        return out
    if epi == EPI_RESID:
        rs = torch.ones(M, 1, dtype=torch.float64) if rowscale is None else f64(rowscale)[torch.arange(M) // rows_per_sample][:, None]
        c = f64(aux) + rs * v
        return {"C": (c, rs.abs() * d + U * (rs * v).abs() + U * c.abs() + TINY)}
    if epi == EPI_DGELU:
        gp, d_gp = gelu_grad(f64(aux))
        c = v * gp
        return {"C": (c, gp.abs() * d + v.abs() * d_gp + U * c.abs() + TINY)}
    if epi == EPI_MULH:
        g = f64(aux)
        c = v * g
        return {"C": (c, g.abs() * d + U * c.abs() + TINY)}
    raise ValueError(epi)


def out_dtype(epi, name, dt):
    """torch dtype of an epilogue's output: fp32 for CARA_EPI_F32 / _RESID, IEEE half for the saved derivative, else the build's"""
    if epi in (EPI_F32, EPI_RESID):
        return torch.float32
    return torch.float16 if (epi == EPI_GELU_DG and name == "C2") else dt


# ----------------------------------------------------------------------------------------------------------------------------
# the products that ride in a launch
# ----------------------------------------------------------------------------------------------------------------------------
def kappa_ts(M):
    """D[k, r] = sum_m X[m, k] G[m, r] and colsum[k] = sum_m X[m, k] after the finishing reduction (cara_tskinny_reduce*): M exact
    products (resp. 16-bit values) meet in ONE sum, whichever way the riders cut it -- tskinny_body's per-wave MFMA chains of 32
    rows a step and its combine through LDS, a slab per wave under helper waves, the epilogue riders' K = 16 MFMAs per row tile
    and their two wave rows (`rv[j][r] + a[r]`), DV's chunks of 32 rows, and the slab reduction's additions in sequence.  A sum
    of M terms has at most M - 1 additions on any path of ANY of these trees (each addition joins two disjoint non-empty sets of
    terms), so kappa_ts = M - 1 bounds every form at once; the chains named above are shorter (M / 32 / waves MFMA steps of 32,
    then waves + slabs additions): kappa_ts_form counts them per form, and the tests hold the device to THAT count; this one is the
    ceiling no form can pass."""
    return max(M - 1, 1)


def kappa_red(n):
    """the finishing reduction over n slabs (strided_sum4 / strided_sum4_v, skinny.hip): four interleaved chains `s0 += p[c]` of
    ceil(n / 4) additions each (they start at 0.f), then (s0 + s1) + (s2 + s3): two more"""
    return -(-n // 4) + 2


def kappa_ts_form(form, M, rows=0, slabs=0):
    """Roundings on the longest path into (one element of D, one column sum), counted per form of the riders -> (kappa_D, kappa_cs).

    "tskinny" (tskinny_body, tskinny_body.h; the products of cara_gemm_with_tskinny_r): steps = ceil(M / 32) K steps are cut into
        nchunks blocks; in a block wave w takes the steps w, w + 4, ...: nm = ceil(ceil(steps / nchunks) / 4) MFMAs 16x16x32 on one
        accumulator (32 roundings each); `s[.] += v[.]` adds the other three waves (3); the reduction runs over nchunks slabs, or,
        where each wave leaves a slab of its own, over 4 nchunks of them (the longer chain is counted).  Column sums: `csum[it] +=
        (float)b[j]` eight times a step (8 nm), then `s += cred[..]` over 4 waves x 4 row groups from 0.f (16), then the reduction.
        nchunks is policy (ts_chunks): the count is the largest over nchunks = 1 .. steps.
    "er" (epilogue_mulh_riders, gemm_epilogue.h, and the ER branch of gemm32_body): a wave's MI = rows / 32 row tiles each add one
        K = 16 MFMA into rv / ru (16 roundings); `rv[j][r] + a[r]` adds the other wave row (1); one slab per row tile of the grid:
        `slabs` of them.  Column sums: per row tile `cs[j] += ((d0 + d1) + (d2 + d3))`, at most 3 additions on a path (3 MI), the two
        shuffles over the row groups (2), the other wave row (1), the reduction.
    "dv" (G8_DV_MMA, gemm8.hip): per 160-row tile five 32-row chunks of two K = 16 MFMAs on accD (160 roundings), one slab per row tile
        and K step, reduced over the `slabs` row tiles.  Column sums: per chunk ((l0 + l1) + (l2 + l3)) + ((h0 + h1) + (h2 + h3)) and
        `accC +=`: at most 4 additions on a path (20), the row groups' combination (at most 4), the reduction."""
    if form == "tskinny":
        steps = -(-M // 32)
        kd = kc = 0
        for nch in range(1, steps + 1):
            nm = -(-(-(-steps // nch)) // 4)
            red = kappa_red(4 * nch)
            kd, kc = max(kd, 32 * nm + 3 + red), max(kc, 8 * nm + 16 + red)
        return kd, kc
    if form == "er":
        mi = rows // 32
        return 16 * mi + 1 + kappa_red(slabs), 3 * mi + 3 + kappa_red(slabs)
    if form == "dv":
        return 160 + kappa_red(slabs), 24 + kappa_red(slabs)
    raise ValueError(form)


def rider_products(X, Gt, M, kappa=None):
    """X [M, K1] 16-bit, Gt [Rp, >= M] 16-bit (columns >= M never read into a sum) -> {"D": (v, d) [K1, Rp], "colsum": (v, d) [K1]}
    with d = gamma(kappa_D) |X|^T |G|, resp. gamma(kappa_cs) sum_m |X|; kappa = kappa_ts_form(...) of the form that ran (None: the
    order-free kappa_ts(M) for both)."""
    X, G = f64(X)[:M], f64(Gt)[:, :M].t()
    kd, kc = kappa if kappa is not None else (kappa_ts(M), kappa_ts(M))
    return {"D": (X.t() @ G, gamma(kd) * (X.abs().t() @ G.abs()) + TINY), "colsum": (X.sum(0), gamma(kc) * X.abs().sum(0) + TINY)}
