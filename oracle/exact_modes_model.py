"""Plain float64 restatement of the kernels of cara_amd/csrc/dropout_exact.hip (weight_dropout = "exact") and
cara_amd/csrc/dense_delta.hip (cp_length 2), each output with a per-element term DERIVED from the kernel's arithmetic, in the
convention of oracle/small_kernels.py (U, gamma, f64, round16, hold_f32, hold_16), oracle/gemm_model.py (kappa_red, TINY) and
oracle/adapter_model.py (s32; d = gamma(kappa) x the same contraction at ABSOLUTE values + 2^-149).

Every function returns (v, d) per output: v the float64 value with a 16-bit rounding exactly where the kernel rounds (the 16-bit
outputs are returned BEFORE their one conversion, which hold_16 performs), d how far the kernel's fp32 value may lie from v.
kappa is the longest chain of roundings on a path into one output element, counted from the code: every fp32 product of an fp32
number is taken as rounded (a contracted fma only removes roundings), a product of two 16-bit operands is exact, an accumulator
that starts at 0.f is counted with every one of its additions.  The fp32 scalars the kernels receive enter as those fp32 numbers:
cara_geom::scale (adapter_model.s32), inv_keep = 1.0f / (1.0f - p) and thresh = (unsigned)((double)(float)p * 2^24)
(mask_params, dropout_exact.hip:204-209).  Nothing here is fitted to a device: tests/test_exact_modes_model.py proves on the host
that an fp32 restatement in another order stays inside every bound and that the slips of tests/exact_modes_common.py do not;
tests/test_exact_modes_contract_gpu.py then holds the device to it.

Sign of zero.  keep_scale(...) * d is 0.f * d on a dropped element: -0.0 for a negative d.  With W == NULL the kernel adds it to
0.f, and 0.f + -0.0 = +0.0: every dropped element of Dm is +0 in BITS (and so is every element of an all-zero adapter, whose sum
starts at 0.f).  With W given, W + (+-0) equals W in VALUE, but a W of -0.0 comes out as +0.0: dropped elements of Weff are held to
W by value, never by bits (hold_16 compares ordinals, in which the two zeros coincide).
"""
import numpy as np
import torch

from cara_amd.dropout import keep_hash_np
from oracle.adapter_model import TINY, s32
from oracle.gemm_model import kappa_red
from oracle.small_kernels import U, gamma, f64, round16, hold_f32, hold_16   # noqa: F401  (re-exported: the two rules)

DD_MAXLK = 192        # dense_delta.hip:20


# --- the mask ---------------------------------------------------------------------------------------------------------------
def mask_params(p):
    """mask_params (dropout_exact.hip:204-209) -> (thresh, inv_keep as the fp32 number) or None where the entry points refuse p"""
    p32 = np.float32(p)
    if not (p32 >= 0 and p32 < 1):
        return None
    return int(float(p32) * 16777216.0), float(np.float32(1.0) / (np.float32(1.0) - p32))


def keep(out, inn, p, seed, lin):
    """bool [out, in]: `(keep_hash(o * in + i, seed, lin) >> 8) >= thresh` (keep_scale, :27-29)"""
    thresh, _ = mask_params(p)
    idx = np.arange(out * inn, dtype=np.uint64).astype(np.uint32)
    return torch.from_numpy(((keep_hash_np(idx, seed, lin) >> np.uint32(8)) >= np.uint32(thresh)).reshape(out, inn))


# --- cara_materialize_merge -------------------------------------------------------------------------------------------------
def kappa_merge(Rp, p, with_w):
    """merge_kernel (:52-56): `d = 0.f; d += v[r] * Us[.][r]` Rp additions of exact products; `keep_scale(...) * d` one product
    (inv_keep is exactly 1.f at p = 0: none); `W + ...` one addition (W == NULL: `0.f + x` is exact)"""
    return Rp + (1 if float(np.float32(p)) != 0.0 else 0) + (1 if with_w else 0)


def merge(W, Um, Vs, p, seed, lin):
    """cara_materialize_merge -> (v, d, keep) with v [out, in] BEFORE the 16-bit rounding: W + keep inv_keep (Vs U^T), W = None
    for the masked delta alone.  Dropped elements: v = W (0 without W) and d = 2^-149 -- the kernel computes W + (+-0)."""
    Vs64, U64 = f64(Vs), f64(Um)
    out, inn, Rp = Vs64.shape[0], U64.shape[0], U64.shape[1]
    _, ik = mask_params(p)
    k = keep(out, inn, p, seed, lin)
    w = f64(W) if W is not None else torch.zeros(out, inn, dtype=torch.float64)
    delta = ik * (Vs64 @ U64.t())
    v = torch.where(k, w + delta, w)
    d = gamma(kappa_merge(Rp, p, W is not None)) * torch.where(k, w.abs() + ik * (Vs64.abs() @ U64.abs().t()), torch.zeros_like(w)) + TINY
    return v, d, k


# --- cara_dropout_grad_contract ---------------------------------------------------------------------------------------------
def kappa_contract(nslab, p, tiles):
    """contract_tile_kernel: the slab sum `a += ...` / slab_sum (:62-66, :93-94) nslab - 1 additions in sequence; `* keep_scale`
    (:96, :100) one product (none at p = 0); `av[j] += gv * u0[j]` (:126-134) the product of an fp32 number and 64 additions per
    tile: 65; reduce_chunks_kernel (:151-167) over `tiles` partials: four interleaved chains of ceil(tiles / 4) additions from 0.f
    and `(s0 + s1) + (s2 + s3)`: kappa_red(tiles)"""
    return (nslab - 1) + (1 if float(np.float32(p)) != 0.0 else 0) + 65 + kappa_red(tiles)


def contract(slabs, Um, Vs, p, seed, lin):
    """cara_dropout_grad_contract on slabs [nslab, out, in] fp32 -> {"dVs": (v, d) [out, Rp], "dU": (v, d) [in, Rp]}:
    dVs = (keep inv_keep sum_z dW_z) U over ceil(in / 64) tiles, dU = (the same)^T Vs over ceil(out / 64) tiles"""
    s64, Vs64, U64 = f64(slabs), f64(Vs), f64(Um)
    nslab, out, inn = s64.shape
    _, ik = mask_params(p)
    k = keep(out, inn, p, seed, lin).double() * ik
    g, ga = k * s64.sum(0), k * s64.abs().sum(0)
    kv, ku = kappa_contract(nslab, p, -(-inn // 64)), kappa_contract(nslab, p, -(-out // 64))
    return {"dVs": (g @ U64, gamma(kv) * (ga @ U64.abs()) + TINY), "dU": (g.t() @ Vs64, gamma(ku) * (ga.t() @ Vs64.abs()) + TINY)}


# --- cara_colsum_bf16 -------------------------------------------------------------------------------------------------------
def colsum_chunk_chain(M, N):
    """the host's policy (:270-272) -> every chunk count the halving loop passes through, the launched one last:
    `chunks = M >= 256 ? ceil(512 * 256 / N) : 1`, at most 256, halved while `chunks > 1 && M / chunks < 16`"""
    chunks = (512 * 256 + N - 1) // N if M >= 256 else 1
    chunks = min(chunks, 256)
    chain = [chunks]
    while chunks > 1 and M // chunks < 16:
        chunks >>= 1
        chain.append(chunks)
    return chain


def colsum_chunks(M, N):
    return colsum_chunk_chain(M, N)[-1]


def colsum_empty_chunks(M, N):
    """chunks whose first row `blockIdx.y * per` (:178) is not below M: they write zeros that reduce_chunks_kernel still adds"""
    chunks = colsum_chunks(M, N)
    per = -(-M // chunks)
    return sum(1 for c in range(chunks) if c * per >= M)


def kappa_colsum(M, chunks):
    """colsum_kernel: the lane's chain `s[j] += x` (:181-190) over its rows m_begin + 2 wave + rp, + 8, ... of a chunk of
    per = ceil(M / chunks) rows: ceil(per / 8) additions; `tsum += part[w][0] + part[w][1]` (:199) the inner sum and four
    additions from 0.f: 5; reduce_chunks_kernel over the chunks: kappa_red(chunks)"""
    per = -(-M // chunks)
    return -(-per // 8) + 5 + kappa_red(chunks)


def colsum(X, M, N):
    """cara_colsum_bf16 -> (v, d, chunks).  The kernel cannot report its chunk count, so kappa is the largest over the counts the
    policy passes through for this (M, N); `chunks` is the one it launches."""
    x = f64(X)[:M, :N]
    chain = colsum_chunk_chain(M, N)
    k = max(kappa_colsum(M, c) for c in chain)
    return x.sum(0), gamma(k) * x.abs().sum(0) + TINY, chain[-1]


# --- cara_dense_delta_materialize / cara_dense_delta_grad --------------------------------------------------------------------
def dd_geom_ok(depth, dim, rank, cp_length=2):
    """dd_geom_ok (dense_delta.hip:156-158)"""
    return cp_length == 2 and depth > 0 and 3 * depth <= DD_MAXLK and dim > 0 and dim % 128 == 0 and 0 < rank <= 64


def kappa_dd_materialize(R):
    """dd_materialize_kernel: `coef = s * R1[r] * A1[...]` (:31) two products; `v[k] += coef[k][r] * x` (:41-44) the product of
    two fp32 numbers and R additions from 0.f"""
    return 2 + 1 + R


def dd_materialize(A1, A2, R1, s, dim):
    """-> (v, d) of Dm [depth, 3 dim, dim] BEFORE the 16-bit rounding: Dm[l][k dim + o][e] = s sum_r R1 A1[3l + k] A2[e dim + o].
    Dmt [depth, dim, 3 dim] is bitwise the transpose per layer (:47-57: the same rounded value goes to both)."""
    s = s32(s)
    a1, a2, r1 = f64(A1), f64(A2), f64(R1)
    depth, R = a1.shape[0] // 3, a1.shape[1]

    def table(a1, a2, r1, s):
        t = ((s * r1 * a1) @ a2.t()).reshape(depth, 3, dim, dim)          # [l][k][e][o]
        return t.permute(0, 1, 3, 2).reshape(depth, 3 * dim, dim)
    return table(a1, a2, r1, s), gamma(kappa_dd_materialize(R)) * table(a1.abs(), a2.abs(), r1.abs(), abs(s)) + TINY


def kappa_dd_grad(depth, dim, R):
    """cara_dense_delta_grad, per kernel (nlk = 3 depth, P = dim^2, nchunk = P / 256):
        dd_grad_a2_kernel: `c = s * R1 * A1` (:66) 2; `acc[r] += cl[r] * d` (:73-79) the product and nlk additions:  nlk + 3
        dd_grad_s_kernel: `d * a[r]` (:101) 1; wave_sum (common.h: `v += __shfl_xor(v, o)` for o = 32 .. 1) six levels: 6;
            `(red[0] + red[1]) + (red[2] + red[3])` (:107) 2:  9 into a chunk partial
        dd_grad_finish_kernel: four interleaved chains over the nchunk partials and `(s0 + s1) + (s2 + s3)` (:118-127): kappa_red(nchunk)
            (dim % 128 == 0 makes P a multiple of 256 and nchunk a multiple of 4: the tail loop at :126 never runs, nor does any
            `p < P` guard of the two kernels above; only the live chain is counted)
            dA1 = `s * R1 * v` (:129) 2 more;  dR1: `acc += A1 * S` (:134) the product and nlk additions, `s * acc` (:135) 1"""
    nlk, nchunk = 3 * depth, dim * dim // 256
    assert nchunk % 4 == 0
    kS = 9 + kappa_red(nchunk)
    return {"A2": nlk + 3, "A1": kS + 2, "R1": kS + 1 + nlk + 1}


def dd_grad(A1, A2, R1, dD, s, dim):
    """-> {"A2": (v, d) [dim^2, R], "A1": (v, d) [3 depth, R], "R1": (v, d) [R]}: the gradient of sum(dD . tensor) with
    tensor[l, k, p] = s sum_r R1 A1[3l + k] A2[p] and dD [depth, 3, dim (e), dim (o)] (p = e dim + o); every monomial has
    coefficient +1, so the contraction at absolute values is the same expression at |.|"""
    s = s32(s)
    a1, a2, r1 = f64(A1), f64(A2), f64(R1)
    depth, R = a1.shape[0] // 3, a1.shape[1]
    dd = f64(dD).reshape(3 * depth, dim * dim)

    def grads(a1, a2, r1, dd, s):
        S = dd @ a2                                                        # [nlk, R]
        return {"A2": dd.t() @ (s * r1 * a1), "A1": s * r1 * S, "R1": s * (a1 * S).sum(0)}
    v, a = grads(a1, a2, r1, dd, s), grads(a1.abs(), a2.abs(), r1.abs(), dd.abs(), abs(s))
    kap = kappa_dd_grad(depth, dim, R)
    return {n: (v[n], gamma(kap[n]) * a[n] + TINY) for n in v}


# --- cara_sum_slabs_f32 -----------------------------------------------------------------------------------------------------
def sum_slabs(slabs, n):
    """dd_sum_slabs_kernel (:144-151) restated in fp32, to be matched BITWISE: two interleaved chains from 0.f over the even and the
    odd slabs, then `s0 + s1`.  slabs [n, count] fp32."""
    x = slabs.detach().float().cpu().numpy()
    s0, s1 = np.zeros_like(x[0]), np.zeros_like(x[0])
    for c in range(0, n - 1, 2):
        s0, s1 = s0 + x[c], s1 + x[c + 1]
    if n % 2:
        s0 = s0 + x[n - 1]
    return torch.from_numpy(s0 + s1)
