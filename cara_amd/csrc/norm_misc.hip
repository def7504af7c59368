// LayerNorm forward/backward and the small pieces of the ViT around the blocks (gfx950 only).
// timm 0.4.12 Block: x = x + drop_path(attn(norm1(x))); x = x + drop_path(mlp(norm2(x)))
// (restated in oracle/cara_oracle.py).  The residual stream stays fp32; normalised activations
// leave as bf16 GEMM operands.  All kernels are HBM-bound streaming passes: one wave per row,
// 16-byte accesses, wave shuffles for the two row reductions.
#include <type_traits>

#include "common.h"

namespace {

// Skinny adapter contraction fused into the kernel that PRODUCES its input (T = X U in
// the forward, G' = dY Vs in the backward; K = C columns, Rp = 32 output columns of which the first `rank`
// are non-zero).  A block of 8 waves normalises 16 rows (2 each), leaves their bf16 images in LDS
// ([16][C + 8]: the 16-byte pad spreads the rows of an MFMA A fragment over the banks), then contracts them
// with Ut [32][C] on the matrix cores: wave w takes the K steps w, w+8, ... (its B fragments come straight
// from global / L2: 1.5 KB per row, the cost of the staging the separate cara_skinny_xu pass pays too), the
// eight partial 16 x 32 tiles are summed through LDS in fixed order.  Two earlier forms were measured and
// dropped: per-lane v_dot2 sums with the factor slice read per row (more L1 traffic than the pass it
// replaces) or held in LDS (as slow as LayerNorm + cara_skinny_xu: ~250 VALU instructions per row).
constexpr int XU_WAVES = 8;         // waves per block of the fused kernels
constexpr int XU_ROWS = 16 / XU_WAVES;   // rows per wave: 16 per block (one MFMA row tile)
// NT = Rp / 16 column tiles of the contraction: 2 (rank <= 32) or 4 (rank <= 64)
template <int V4, int NT = 2>
struct XuLds {
  static constexpr int LDY = V4 * 256 + 8;   // bf16 elements per staged row
  bf16 y[16 * LDY];
  float part[XU_WAVES][NT][64 * 4];
};
// the block's 16 staged bf16 rows -> K-panel-major global image [C/32][yp][32]: a wave writes one panel's 16 rows
// (16 x 64 B = one contiguous KiB of full cache lines) per instruction, instead of each row's 8-byte pieces
// scattered over C/32 panels.  Call after the rows are complete (a __syncthreads() away from the staging).
template <int V4, int NT>
__device__ __forceinline__ void panel_store(const XuLds<V4, NT>& L, bf16* __restrict__ y, const int yp, const int row_base, const int M) {
  constexpr int C = V4 * 256, LDY = XuLds<V4, NT>::LDY;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = lane >> 2, chunk = lane & 3;
  if (row_base + row >= M) return;
#pragma unroll
  for (int p = wave; p < C / 32; p += XU_WAVES)
    *reinterpret_cast<bf16x8*>(y + ((size_t)p * yp + row_base + row) * 32 + chunk * 8) =
        *reinterpret_cast<const bf16x8*>(L.y + row * LDY + p * 32 + chunk * 8);
}
// a wave's B fragments of the contraction (its K steps wave, wave + 8, ...: C/256 of them, two column tiles each):
// requested at the top of the kernel so that their L2 latency passes under the row loads and reductions
template <int V4, int NT = 2>
struct UtFrags {
  bf16x8 u[V4][NT];
};
template <int V4, int NT>
__device__ __forceinline__ UtFrags<V4, NT> load_ut_frags(const bf16* __restrict__ Ut) {
  constexpr int C = V4 * 256;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  UtFrags<V4, NT> f;
#pragma unroll
  for (int k = 0; k < V4; ++k)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      f.u[k][nt] = *reinterpret_cast<const bf16x8*>(Ut + (size_t)(nt * 16 + fr) * C + (wave + k * XU_WAVES) * 32 + fq * 8);
  return f;
}
template <int V4, int NT>
__device__ __forceinline__ void block_contract(XuLds<V4, NT>& L, const UtFrags<V4, NT>& uf, bf16* __restrict__ T,
                                               bf16* __restrict__ Tt, const int ldt, const int row_base, const int M, const int Rp) {
  constexpr int LDY = XuLds<V4, NT>::LDY;
  static_assert(XU_WAVES == 8, "K steps per wave = C / 32 / 8 = V4");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  __syncthreads();   // the 16 staged rows are complete
  f32x4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < V4; ++k) {
    const int s = wave + k * XU_WAVES;
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(L.y + fr * LDY + s * 32 + fq * 8);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, uf.u[k][nt], acc[nt], 0, 0, 0);
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) *reinterpret_cast<f32x4*>(&L.part[wave][nt][lane * 4]) = acc[nt];
  __syncthreads();
  if (wave < NT) {   // wave nt sums column tile nt: lane (fr, fq) holds rows fq*4 .. +3 of column nt*16 + fr
    const int nt = wave;
    f32x4 t = *reinterpret_cast<const f32x4*>(&L.part[0][nt][lane * 4]);
#pragma unroll
    for (int w = 1; w < XU_WAVES; ++w) t += *reinterpret_cast<const f32x4*>(&L.part[w][nt][lane * 4]);
    const int col = nt * 16 + fr, m0 = row_base + fq * 4;
    const bf16x4 o = {(bf16)t[0], (bf16)t[1], (bf16)t[2], (bf16)t[3]};
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (m0 + r < M) T[(size_t)(m0 + r) * Rp + col] = o[r];
    if (Tt) {
      if (m0 + 4 <= M) {
        *reinterpret_cast<bf16x4*>(Tt + (size_t)col * ldt + m0) = o;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (m0 + r < M) Tt[(size_t)col * ldt + m0 + r] = o[r];
      }
    }
  }
  else if (wave < Rp / 16) {
    // NT * 16 < Rp (rank <= 16 at Rp = 32: only the first column tile is computed, the rows of Ut beyond the rank are
    // zero): the tiles that were skipped are written as the zeros they are
    const int col = wave * 16 + fr, m0 = row_base + fq * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (m0 + r >= M) continue;
      T[(size_t)(m0 + r) * Rp + col] = (bf16)0.f;
      if (Tt) Tt[(size_t)col * ldt + m0 + r] = (bf16)0.f;
    }
  }
}

template <int V4, bool XU, int NT = 2>  // V4 = C / 256 : float4 per lane; XU: fused contraction, XU_ROWS rows per wave
__global__ __launch_bounds__(XU ? XU_WAVES * 64 : 256) void ln_fwd_kernel(const float* __restrict__ x, long ldx,
                                                     const float* __restrict__ gamma,
                                                     const float* __restrict__ beta,
                                                     bf16* __restrict__ y, float* __restrict__ mean,
                                                     float* __restrict__ rstd, int M, float eps,
                                                     const bf16* __restrict__ Ut, int rank, int Rp, bf16* __restrict__ T,
                                                     bf16* __restrict__ Tt, int ldt, const int yp) {
  constexpr int C = V4 * 256;
  constexpr int RPW = XU ? XU_ROWS : 1;
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * (XU ? XU_WAVES : 4) + (threadIdx.x >> 6)) * RPW;
  __shared__ __attribute__((aligned(16))) XuLds<XU ? V4 : 0, XU ? NT : 1> L;
  // (NT = 4: twice the fragments; they are requested behind the row loop, as in the backward kernel, so that the kernel
  // keeps its occupancy)
  UtFrags<XU ? V4 : 1, XU ? NT : 1> uf;
  if constexpr (XU && NT <= 2) uf = load_ut_frags<V4, NT>(Ut);
  // all of a wave's rows are requested before anything is reduced: a wave keeps RPW x V4 16-byte loads in flight
  // instead of V4 (the kernel is latency-bound: one row at a time reached 3.4 TB/s)
  float4 v[RPW][V4];
#pragma unroll
  for (int rr = 0; rr < RPW; ++rr) {
    const int row = row0 + rr < M ? row0 + rr : M - 1;
    const float* xr = x + (size_t)row * ldx;
#pragma unroll
    for (int i = 0; i < V4; ++i) v[rr][i] = *reinterpret_cast<const float4*>(xr + i * 256 + lane * 4);
  }
  float4 gm[V4], bt[V4];
#pragma unroll
  for (int i = 0; i < V4; ++i) {
    gm[i] = *reinterpret_cast<const float4*>(gamma + i * 256 + lane * 4);
    bt[i] = *reinterpret_cast<const float4*>(beta + i * 256 + lane * 4);
  }
#pragma unroll
  for (int rr = 0; rr < RPW; ++rr) {
  const int row = row0 + rr;
  if (row >= M) break;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < V4; ++i) s += (v[rr][i].x + v[rr][i].y) + (v[rr][i].z + v[rr][i].w);
  const float mu = wave_sum(s) * (1.0f / C);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < V4; ++i) {
    const float a = v[rr][i].x - mu, b = v[rr][i].y - mu, c = v[rr][i].z - mu, d = v[rr][i].w - mu;
    q += (a * a + b * b) + (c * c + d * d);
  }
  const float rs = rsqrtf(wave_sum(q) * (1.0f / C) + eps);
  bf16* yr = y + (size_t)row * C;
  bf16x4 yb[V4];
#pragma unroll
  for (int i = 0; i < V4; ++i) {
    const int c0 = i * 256 + lane * 4;
    const float4 g = gm[i];
    const float4 b = bt[i];
    bf16x4 o = {(bf16)((v[rr][i].x - mu) * rs * g.x + b.x), (bf16)((v[rr][i].y - mu) * rs * g.y + b.y),
                (bf16)((v[rr][i].z - mu) * rs * g.z + b.z), (bf16)((v[rr][i].w - mu) * rs * g.w + b.w)};
    // yp > 0: y as K-panel-major [C/32][yp][32] (the A operand layout of the GEMM that reads it)
    if (!(XU && yp))   // (fused kernels write the panel image from the staged rows, panel_store)
      *reinterpret_cast<bf16x4*>(yp ? y + ((size_t)(c0 >> 5) * yp + row) * 32 + (c0 & 31) : yr + c0) = o;
    yb[i] = o;
  }
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
  if constexpr (XU) {
#pragma unroll
    for (int i = 0; i < V4; ++i)
      *reinterpret_cast<bf16x4*>(L.y + (row - blockIdx.x * 16) * XuLds<V4, NT>::LDY + i * 256 + lane * 4) = yb[i];
  }
  }
  if constexpr (XU) {
    if (yp) {
      __syncthreads();
      panel_store<V4, NT>(L, y, yp, blockIdx.x * 16, M);
    }
    if constexpr (NT > 2) uf = load_ut_frags<V4, NT>(Ut);
    block_contract<V4, NT>(L, uf, T, Tt, ldt, blockIdx.x * 16, M, Rp);   // T = LN(x) U of the next linear
  }
}

// dx = rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma,  xhat = (x - mu) * rstd
template <int V4, bool XU, int NT = 2>
__global__ __launch_bounds__(XU ? XU_WAVES * 64 : 256) void ln_bwd_kernel(const bf16* __restrict__ dy, const float* __restrict__ x,
                                                     long ldx, const float* __restrict__ gamma,
                                                     const float* __restrict__ mean,
                                                     const float* __restrict__ rstd,
                                                     const float* __restrict__ dx_in,
                                                     float* __restrict__ dx_out, bf16* __restrict__ dyb,
                                                     const float* __restrict__ rowscale,
                                                     int rows_per_sample, int M,
                                                     const bf16* __restrict__ Vst, int rank, int Rp, bf16* __restrict__ G,
                                                     bf16* __restrict__ Gt, int ldt, const int yp, const int dx_in_every) {
  // dx_in_every > 0: the running gradient dx_in is nonzero on rows that are multiples of it only (the last block of a ViT whose head
  // reads the cls token: gradient has reached nothing but the cls rows yet) -- the other rows are neither read nor expected zeroed
  constexpr int C = V4 * 256;
  constexpr int RPW = XU ? XU_ROWS : 1;
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * (XU ? XU_WAVES : 4) + (threadIdx.x >> 6)) * RPW;
  __shared__ __attribute__((aligned(16))) XuLds<XU ? V4 : 0, XU ? NT : 1> L;
  // Every load of the wave's rows -- x, dy AND the running gradient dx_in, which the second half of a row's work reads -- is
  // requested before anything is reduced: one memory latency per wave instead of two per row (the kernel is one round of
  // waves, all in the same phase: nothing else hides a dependent load)
  float4 xv[RPW][V4], pv[RPW][V4];
  bf16x4 dv[RPW][V4];
  float mu_[RPW], rs_[RPW];
#pragma unroll
  for (int rr = 0; rr < RPW; ++rr) {
    const int row = row0 + rr < M ? row0 + rr : M - 1;
    const float* xr = x + (size_t)row * ldx;
    const bf16* dr = dy + (size_t)row * C;
#pragma unroll
    for (int i = 0; i < V4; ++i) {
      xv[rr][i] = *reinterpret_cast<const float4*>(xr + i * 256 + lane * 4);
      dv[rr][i] = *reinterpret_cast<const bf16x4*>(dr + i * 256 + lane * 4);
    }
    mu_[rr] = mean[row];
    rs_[rr] = rstd[row];
  }
  bool has_in[RPW];
#pragma unroll
  for (int rr = 0; rr < RPW; ++rr) {
    const int row = row0 + rr < M ? row0 + rr : M - 1;
    has_in[rr] = dx_in && (dx_in_every <= 0 || row % dx_in_every == 0);   // (wave-uniform: a wave owns whole rows)
    if (has_in[rr]) {
#pragma unroll
      for (int i = 0; i < V4; ++i) pv[rr][i] = *reinterpret_cast<const float4*>(dx_in + (size_t)row * ldx + i * 256 + lane * 4);
    }
  }
  float4 gmv[V4];
#pragma unroll
  for (int i = 0; i < V4; ++i) gmv[i] = *reinterpret_cast<const float4*>(gamma + i * 256 + lane * 4);
#pragma unroll
  for (int rr = 0; rr < RPW; ++rr) {
  const int row = row0 + rr;
  if (row >= M) break;
  const float mu = mu_[rr], rs = rs_[rr];
  float4 g[V4], xh[V4];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < V4; ++i) {
    const float4 xq = xv[rr][i];
    const float4 gm = gmv[i];
    const bf16x4 d = dv[rr][i];
    xh[i] = make_float4((xq.x - mu) * rs, (xq.y - mu) * rs, (xq.z - mu) * rs, (xq.w - mu) * rs);
    g[i] = make_float4((float)d[0] * gm.x, (float)d[1] * gm.y, (float)d[2] * gm.z, (float)d[3] * gm.w);
    s1 += (g[i].x + g[i].y) + (g[i].z + g[i].w);
    s2 += (g[i].x * xh[i].x + g[i].y * xh[i].y) + (g[i].z * xh[i].z + g[i].w * xh[i].w);
  }
  const float c1 = wave_sum(s1) * (1.0f / C), c2 = wave_sum(s2) * (1.0f / C);
  const float sc = rowscale ? rowscale[row / rows_per_sample] : 1.f;
  float* dor = dx_out + (size_t)row * ldx;
  bf16* db = dyb ? dyb + (size_t)row * ldx : nullptr;
  bf16x4 yb[V4];
#pragma unroll
  for (int i = 0; i < V4; ++i) {
    const int c0 = i * 256 + lane * 4;
    float4 o = make_float4(rs * (g[i].x - c1 - xh[i].x * c2), rs * (g[i].y - c1 - xh[i].y * c2),
                           rs * (g[i].z - c1 - xh[i].z * c2), rs * (g[i].w - c1 - xh[i].w * c2));
    if (has_in[rr]) {
      const float4 pq = pv[rr][i];
      o.x += pq.x; o.y += pq.y; o.z += pq.z; o.w += pq.w;
    }
    *reinterpret_cast<float4*>(dor + c0) = o;
    float4 os = make_float4(o.x * sc, o.y * sc, o.z * sc, o.w * sc);
#ifdef CARA_F16_OPERANDS
    // IEEE-half build: the compiler folds product + conversion into v_fma_mixlo_f16 (ONE rounding of the exact product) in some
    // instantiations and keeps v_mul_f32 + v_cvt_f16_f32 (two) in others, so the fused and the plain kernels disagreed on dyb
    // where the fp32 product lands on a half tie (tests/test_small_kernels_gpu.py).  The product is an fp32 value everywhere:
    asm volatile("" : "+v"(os.x), "+v"(os.y), "+v"(os.z), "+v"(os.w));
#endif
    bf16x4 b = {(bf16)os.x, (bf16)os.y, (bf16)os.z, (bf16)os.w};
    if (db && !(XU && yp)) *reinterpret_cast<bf16x4*>(yp ? dyb + ((size_t)(c0 >> 5) * yp + row) * 32 + (c0 & 31) : db + c0) = b;
    yb[i] = b;
  }
  if constexpr (XU) {
#pragma unroll
    for (int i = 0; i < V4; ++i)
      *reinterpret_cast<bf16x4*>(L.y + (row - blockIdx.x * 16) * XuLds<V4, NT>::LDY + i * 256 + lane * 4) = yb[i];
  }
  }
  if constexpr (XU) {
    if (yp) {
      __syncthreads();
      panel_store<V4, NT>(L, dyb, yp, blockIdx.x * 16, M);
    }
    // (the B fragments are requested here, not at the top: holding them through the row loop costs the backward kernel a
    // workgroup of occupancy -- 138 VGPRs, 36 us instead of 31)
    block_contract<V4, NT>(L, load_ut_frags<V4, NT>(Vst), G, Gt, ldt, blockIdx.x * 16, M, Rp);   // G' = dY Vs of the linear below
  }
}

__global__ __launch_bounds__(256) void assemble_kernel(const float* __restrict__ emb, const float* __restrict__ cls,
                                                       const float* __restrict__ pos, float* __restrict__ x,
                                                       int B, int P, int D, long total4) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total4) return;
  const long e = idx * 4;
  const int d = (int)(e % D);
  const long tok = e / D;
  const int t = (int)(tok % (P + 1)), b = (int)(tok / (P + 1));
  const float4 pv = *reinterpret_cast<const float4*>(pos + (size_t)t * D + d);
  float4 s = (t == 0) ? *reinterpret_cast<const float4*>(cls + d)
                      : *reinterpret_cast<const float4*>(emb + ((size_t)b * P + (t - 1)) * D + d);
  s.x += pv.x; s.y += pv.y; s.z += pv.z; s.w += pv.w;
  *reinterpret_cast<float4*>(x + e) = s;
}

// assemble_kernel behind a patch dropout: token 1 + j of sample b is kept patch keep[b][j], whose position row is 1 + keep[b][j] of
// the full table pos [1 + P, D].  An entry outside [0, P) reads no position row: the token is emb's row alone.
__global__ __launch_bounds__(256) void assemble_keep_kernel(const float* __restrict__ emb, const float* __restrict__ cls,
                                                            const float* __restrict__ pos, const int* __restrict__ keep,
                                                            float* __restrict__ x, int B, int K, int P, int D, long total4) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total4) return;
  const long e = idx * 4;
  const int d = (int)(e % D);
  const long tok = e / D;
  const int t = (int)(tok % (K + 1)), b = (int)(tok / (K + 1));
  const int pr = t == 0 ? -1 : keep[(size_t)b * K + (t - 1)];
  const bool has_pos = t == 0 || (pr >= 0 && pr < P);
  float4 s = (t == 0) ? *reinterpret_cast<const float4*>(cls + d)
                      : *reinterpret_cast<const float4*>(emb + ((size_t)b * K + (t - 1)) * D + d);
  if (has_pos) {
    const float4 pv = *reinterpret_cast<const float4*>(pos + (size_t)(t == 0 ? 0 : 1 + pr) * D + d);
    s.x += pv.x; s.y += pv.y; s.z += pv.z; s.w += pv.w;
  }
  *reinterpret_cast<float4*>(x + e) = s;
}

// one wave per sample; loss = mean_b (lse_b - logit_b[y_b]); dlogits = (softmax - onehot) / B
// A label outside [0, C) (torch's ignore index -100, a split with more classes than the head, an int64 that only its low
// 32 bits would bring into range) never indexes the row: that sample's loss term and its dlogits row are NaN, so the mean
// loss is NaN too and the step is visibly wrong instead of quietly so.  Every other sample's outputs are unaffected.
__global__ __launch_bounds__(64) void xent_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                  float* __restrict__ loss_per, float* __restrict__ dlogits,
                                                  int B, int C, float dscale, const float* __restrict__ loss_scale) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* lr = logits + (size_t)b * C;
  float m = -3.0e38f;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, lr[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += __expf(lr[c] - m);
  s = wave_sum(s);
  const float lse = m + __logf(s);
  const int64_t yl = labels[b];
  const bool ok = yl >= 0 && yl < C;   // (wave-uniform)
  const int y = ok ? (int)yl : 0;
  const float qnan = __builtin_nanf("");
  const float invB = 1.0f / B;
  // (the gradient's scale: 1/B of the mean, times 1/world of a data-parallel job, times the loss scale of the IEEE-half build)
  const float gsc = invB * dscale * (loss_scale ? *loss_scale : 1.f);
  if (dlogits)
    for (int c = lane; c < C; c += 64)
      dlogits[(size_t)b * C + c] = ok ? (__expf(lr[c] - lse) - (c == y ? 1.f : 0.f)) * gsc : qnan;
  if (lane == 0) loss_per[b] = ok ? (lse - lr[y]) * invB : qnan;
}
// xent_kernel against a soft target (label smoothing eps; Mixup / CutMix: the partner's label with weight t = the fp32 whose bits
// mix[b][6] holds; mix NULL: t = 0):  q_c = (1 - eps) ((1 - t) [c == ya] + t [c == yb]) + eps / C,  ya = labels[b], yb =
// labels[partner],  term_b = (lse_b - sum_c q_c l_c) / B,  dlogits = (softmax - q) gsc.  sum_c q_c l_c = (1 - eps) (l_ya + t (l_yb -
// l_ya)) + (eps / C) sum_c l_c: one more wave reduction, its sum gathered in the pass that finds the maximum.  The lerp is exact at
// t == 0 and where ya == yb, 1 - eps is 1 at eps == 0 and the eps / C term is added only where it is not zero: eps == 0 && t == 0
// gives q == the one-hot and every output bit for bit xent_kernel's.
// Guards as there: ya or yb outside [0, C), partner outside [0, B) (checked before labels[partner] is formed) or a t that is not
// in [0, 1] (a NaN fails t >= 0) index nothing and make the sample's term and dlogits row NaN; other samples are unaffected.
__global__ __launch_bounds__(64) void xent_mix_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                      const int* __restrict__ mix, float eps, float* __restrict__ loss_per,
                                                      float* __restrict__ dlogits, int B, int C, float dscale,
                                                      const float* __restrict__ loss_scale) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* lr = logits + (size_t)b * C;
  float m = -3.0e38f, sl = 0.f;
  for (int c = lane; c < C; c += 64) {
    m = fmaxf(m, lr[c]);
    sl += lr[c];
  }
  m = wave_max(m);
  sl = wave_sum(sl);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += __expf(lr[c] - m);
  s = wave_sum(s);
  const float lse = m + __logf(s);
  const int partner = mix ? mix[(size_t)b * 8] : b;
  const float t = mix ? __int_as_float(mix[(size_t)b * 8 + 6]) : 0.f;
  const int64_t yal = labels[b];
  const bool pok = partner >= 0 && partner < B;
  const int64_t ybl = pok ? labels[partner] : -1;
  const bool ok = yal >= 0 && yal < C && ybl >= 0 && ybl < C && t >= 0.f && t <= 1.f;   // (wave-uniform)
  const int ya = ok ? (int)yal : 0, yb = ok ? (int)ybl : 0;
  const float wa = (1.f - eps) * (1.f - t), wb = (1.f - eps) * t, u = eps / (float)C;
  const float qnan = __builtin_nanf("");
  const float invB = 1.0f / B;
  const float gsc = invB * dscale * (loss_scale ? *loss_scale : 1.f);   // (xent_kernel's)
  if (dlogits)
    for (int c = lane; c < C; c += 64) {
      const float q = (c == ya ? wa : 0.f) + (c == yb ? wb : 0.f) + u;
      dlogits[(size_t)b * C + c] = ok ? (__expf(lr[c] - lse) - q) * gsc : qnan;
    }
  if (lane == 0) {
    const float la = lr[ya];
    float dot = (1.f - eps) * (la + t * (lr[yb] - la));
    if (u != 0.f) dot += u * sl;
    loss_per[b] = ok ? (lse - dot) * invB : qnan;
  }
}
// xent_mix_kernel with a weight per class and a bias on the logits (cw, cb fp32 [C]; NULL: all ones / all zeros):  z_c = l_c + cb_c
// (the softmax, lse and p are of z),  W_b = sum_c cw_c q_c,  term_b = (W_b lse_b - sum_c cw_c q_c z_c) / B,  dlogits = (p_c W_b - cw_c q_c)
// gsc: torch's cross_entropy(l + cb, q, weight=cw, reduction="sum") / B.  With q of xent_mix_kernel,  W_b = wa cw_ya + wb cw_yb + (eps / C)
// sum_c cw_c  and  sum_c cw_c q_c z_c = wa cw_ya z_ya + wb cw_yb z_yb + (eps / C) sum_c cw_c z_c: two more wave reductions, gathered in the
// pass that finds the maximum, and the two gathers of xent_mix_kernel; the eps / C terms are added only where they are not zero.
// Guards as there; a guarded sample gathers class 0 of cw and cb, never a class its labels name.  The values of cw and cb are not
// looked at: the caller keeps cw finite and >= 0 and cb finite.
__global__ __launch_bounds__(64) void xent_bal_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                      const int* __restrict__ mix, float eps, const float* __restrict__ cw,
                                                      const float* __restrict__ cb, float* __restrict__ loss_per,
                                                      float* __restrict__ dlogits, int B, int C, float dscale,
                                                      const float* __restrict__ loss_scale) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* lr = logits + (size_t)b * C;
  float m = -3.0e38f, sw = 0.f, swz = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float z = cb ? lr[c] + cb[c] : lr[c], w = cw ? cw[c] : 1.f;
    m = fmaxf(m, z);
    sw += w;
    swz += w * z;
  }
  m = wave_max(m);
  sw = wave_sum(sw);
  swz = wave_sum(swz);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += __expf((cb ? lr[c] + cb[c] : lr[c]) - m);
  s = wave_sum(s);
  const float lse = m + __logf(s);
  const int partner = mix ? mix[(size_t)b * 8] : b;
  const float t = mix ? __int_as_float(mix[(size_t)b * 8 + 6]) : 0.f;
  const int64_t yal = labels[b];
  const bool pok = partner >= 0 && partner < B;
  const int64_t ybl = pok ? labels[partner] : -1;
  const bool ok = yal >= 0 && yal < C && ybl >= 0 && ybl < C && t >= 0.f && t <= 1.f;   // (wave-uniform)
  const int ya = ok ? (int)yal : 0, yb = ok ? (int)ybl : 0;
  const float wa = (1.f - eps) * (1.f - t), wb = (1.f - eps) * t, u = eps / (float)C;
  const float ga = cw ? cw[ya] : 1.f, gb = cw ? cw[yb] : 1.f;
  float W = wa * ga + wb * gb;
  if (u != 0.f) W += u * sw;
  const float qnan = __builtin_nanf("");
  const float invB = 1.0f / B;
  const float gsc = invB * dscale * (loss_scale ? *loss_scale : 1.f);   // (xent_kernel's)
  if (dlogits)
    for (int c = lane; c < C; c += 64) {
      const float z = cb ? lr[c] + cb[c] : lr[c], w = cw ? cw[c] : 1.f;
      const float q = (c == ya ? wa : 0.f) + (c == yb ? wb : 0.f) + u;
      dlogits[(size_t)b * C + c] = ok ? (__expf(z - lse) * W - w * q) * gsc : qnan;
    }
  if (lane == 0) {
    const float za = cb ? lr[ya] + cb[ya] : lr[ya], zb = cb ? lr[yb] + cb[yb] : lr[yb];
    float dot = wa * (ga * za) + wb * (gb * zb);
    if (u != 0.f) dot += u * swz;
    loss_per[b] = ok ? (W * lse - dot) * invB : qnan;
  }
}
// The sigmoid family on xent_mix_kernel's soft target: per element (b, c), z = logits[b][c], q = q_c of xent_mix_kernel (the same
// wa, wb, u and guards), with a threshold thr >= 0 replaced by (q > thr ? 1 : 0) -- timm's target.gt(thr), decided on the fp32 q.
// Everything comes from ONE exponential that cannot overflow, e = __expf(-|z|) in [0, 1], and w = 1 + e in [1, 2]:
//   L = log1p(e) = __logf(w) (e / (w - 1)), or e where w == 1: w - 1 is exact, and log(w) / (w - 1) barely moves when 1 + e rounds to
//   w, so L keeps its RELATIVE accuracy down to the smallest e -- __logf(1 + e) alone is off by u absolutely, 1e-3 of L at |z| = 9,
//   which the focal loss multiplies into the gradient of every easy negative;
//   sp(z) = max(z, 0) + L,  sp(-z) = max(-z, 0) + L  (softplus; -log sigma(-z) and -log sigma(z)),
//   r = 1 / w,  sigma(|z|) = r,  sigma(-|z|) = e r:  s+ = sigma(z) and s- = sigma(-z) are these two in the order of z's sign --
// neither is formed as 1 - the other.  The difference s+ - q is formed as (1 - q) s+ - q s- (s+ + s- = 1), a difference of two
// non-negative products of which one is zero for a hard target: no cancellation at a saturated logit.
// BCE (FOCAL = false):  l = (pw q) sp(-z) + (1 - q) sp(z),  dl/dz = (1 - q) s+ - (pw q) s-  [= s+ (1 - q + pw q) - pw q];  pw =
//   pos_weight[c] or 1 -- torch's binary_cross_entropy_with_logits(z, q, pos_weight = pw).  A product with 1.f is exact: a vector of
//   ones gives the bits of no vector.
// Focal (FOCAL = true; torchvision's sigmoid_focal_loss on a soft q):  ce = q sp(-z) + (1 - q) sp(z),  m = q s- + (1 - q) s+ (a sum
//   of non-negative terms),  a = alpha q + (1 - alpha)(1 - q) or 1,  l = a m^g ce,
//   dl/dz = a [((1 - q) s+ - q s-) m^g + g ce m^(g - 1) s+ s- (1 - 2 q)].   m^(g - 1) is 1 at g == 1, m at g == 2 and
//   __expf((g - 1) __logf(m)) for another g > 1 (0 at m == 0);  m^g = m^(g - 1) m;  g == 0 takes m^g = 1 and no second term.
// term_b = (sum_c l) invBD,  invBD = the fp32 nearest to 1 / (B D), D = C (the mean over the classes) or 1 (their sum);
// dlogits = dl/dz gsc,  gsc = invBD dscale loss scale.  One wave per sample, classes lane-strided, one pass; the loss does not depend
// on whether dlogits is written.  Plain operators, no contraction: the bound of tests/sigmoid_loss_model.py counts every rounding.
// Guards as in xent_mix_kernel; pos_weight is read by class index c only, never through a label.
template <bool FOCAL>
__global__ __launch_bounds__(64) void sigmoid_loss_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                          const int* __restrict__ mix, float eps, float thr, float fg, float alpha,
                                                          const float* __restrict__ pw, float* __restrict__ loss_per,
                                                          float* __restrict__ dlogits, int B, int C, float invBD, float dscale,
                                                          const float* __restrict__ loss_scale) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* lr = logits + (size_t)b * C;
  const int partner = mix ? mix[(size_t)b * 8] : b;
  const float t = mix ? __int_as_float(mix[(size_t)b * 8 + 6]) : 0.f;
  const int64_t yal = labels[b];
  const bool pok = partner >= 0 && partner < B;
  const int64_t ybl = pok ? labels[partner] : -1;
  const bool ok = yal >= 0 && yal < C && ybl >= 0 && ybl < C && t >= 0.f && t <= 1.f;   // (wave-uniform)
  const int ya = ok ? (int)yal : 0, yb = ok ? (int)ybl : 0;
  const float wa = (1.f - eps) * (1.f - t), wb = (1.f - eps) * t, u = eps / (float)C;   // (xent_mix_kernel's)
  const float qnan = __builtin_nanf("");
  const float gsc = invBD * dscale * (loss_scale ? *loss_scale : 1.f);
  const float g1 = fg - 1.f, oma = 1.f - alpha;
  float sl = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float z = lr[c];
    float q = (c == ya ? wa : 0.f) + (c == yb ? wb : 0.f) + u;
    if (thr >= 0.f) q = q > thr ? 1.f : 0.f;
    const float omq = 1.f - q;
    const float e = __expf(-fabsf(z)), w = 1.f + e, r = 1.f / w, er = e * r;
    const float L = w == 1.f ? e : __logf(w) * (e / (w - 1.f));
    const bool pos = z >= 0.f;
    const float sp = pos ? r : er, sm = pos ? er : r;                 // sigma(z), sigma(-z)
    const float spz = fmaxf(z, 0.f) + L, spn = fmaxf(-z, 0.f) + L;    // softplus(z), softplus(-z)
    float l, g;
    if (!FOCAL) {
      const float pq = (pw ? pw[c] : 1.f) * q;
      l = pq * spn + omq * spz;
      g = omq * sp - pq * sm;
    } else {
      const float ce = q * spn + omq * spz;
      const float m = q * sm + omq * sp;
      const float d0 = omq * sp - q * sm;
      if (fg == 0.f) {
        l = ce;
        g = d0;
      } else {
        const float mg1 = fg == 1.f ? 1.f : fg == 2.f ? m : __expf(g1 * __logf(m));
        const float mg = mg1 * m;
        l = mg * ce;
        g = d0 * mg + fg * ce * mg1 * (sp * sm) * (1.f - 2.f * q);
      }
      if (alpha >= 0.f) {
        const float a = alpha * q + oma * omq;
        l = a * l;
        g = a * g;
      }
    }
    sl += l;
    if (dlogits) dlogits[(size_t)b * C + c] = ok ? g * gsc : qnan;
  }
  sl = wave_sum(sl);
  if (lane == 0) loss_per[b] = ok ? sl * invBD : qnan;
}
// Knowledge distillation on xent_mix_kernel's soft target q (the same wa, wb, u and guards): z = the student's row, t = the teacher's
// row (fp32, no gradient), a = alpha in (0, 1], T = temperature.  invT = 1 / T is formed once and every tempered logit is x invT.
// tempered_lse(x, invT) = m + __logf(sum_c __expf(x_c invT - m)), m = max_c x_c invT, is the ONE device function behind the three
// log-sum-exps -- lse(z) (invT = 1: a product with 1.f is exact), lse(z / T) and lse(t / T) -- so that the student's and the
// teacher's tempered log-probabilities  lz_c = z_c invT - lse(z / T),  lt_c = t_c invT - lse(t / T)  are the same operations on
// either row:  pT = __expf(lz), r = __expf(lt), and a teacher row equal to the student's gives pT - r == 0 and lt - lz == 0 exactly.
// soft (HARD = false):  kl = sum_c r_c (lt_c - lz_c) -- the log-ratio form: shift-invariant in either row, its error scales with the
//   teacher's entropy and cross-entropy and not with the size of the logits, and it reuses lz and lt, which the gradient exponentiates
//   anyway;  term_b = ((1 - a) (lse - dot) + (a T T) kl) invB,  dlogits = ((1 - a) (p - q) + (a T) (pT - r)) gsc,  p = __expf(z - lse);
//   dot = sum_c q_c z_c as xent_mix_kernel forms it.
// hard (HARD = true; DeiT):  yt = the LOWEST class that attains the teacher row's maximum (cara_eval_accumulate's tie rule),
//   q' = (1 - a) q + a [c == yt]:  term_b = (lse - ((1 - a) dot + a z_yt)) invB,  dlogits = (p - q') gsc;  T is not read.
// A teacher row with any non-finite value (found by |t_c| <= FLT_MAX, which a NaN fails, before anything else looks at the row)
// joins the label guards: the term and the dlogits row are NaN and yt is 0, never an index formed from such a row.  The loss does
// not depend on whether dlogits is written.  Plain operators, no contraction: the bound of tests/distill_model.py counts every rounding.
__device__ __forceinline__ float tempered_lse(const float* __restrict__ row, int C, int lane, float invT) {
#pragma clang fp contract(off)
  float m = -3.0e38f;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, row[c] * invT);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += __expf(row[c] * invT - m);
  s = wave_sum(s);
  return m + __logf(s);
}
template <bool HARD>
__global__ __launch_bounds__(64) void distill_kernel(const float* __restrict__ logits, const float* __restrict__ teacher,
                                                     const int64_t* __restrict__ labels, const int* __restrict__ mix, float eps,
                                                     float alpha, float T, float* __restrict__ loss_per, float* __restrict__ dlogits,
                                                     int B, int C, float dscale, const float* __restrict__ loss_scale) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* lr = logits + (size_t)b * C;
  const float* tr = teacher + (size_t)b * C;
  float sl = 0.f, tbad = 0.f;
  for (int c = lane; c < C; c += 64) {
    sl += lr[c];
    if (!(fabsf(tr[c]) <= 3.4028235e38f)) tbad = 1.f;
  }
  sl = wave_sum(sl);
  tbad = wave_max(tbad);
  const float lse = tempered_lse(lr, C, lane, 1.f);
  const int partner = mix ? mix[(size_t)b * 8] : b;
  const float t = mix ? __int_as_float(mix[(size_t)b * 8 + 6]) : 0.f;
  const int64_t yal = labels[b];
  const bool pok = partner >= 0 && partner < B;
  const int64_t ybl = pok ? labels[partner] : -1;
  const bool ok = yal >= 0 && yal < C && ybl >= 0 && ybl < C && t >= 0.f && t <= 1.f && tbad == 0.f;   // (wave-uniform)
  const int ya = ok ? (int)yal : 0, yb = ok ? (int)ybl : 0;
  const float wa = (1.f - eps) * (1.f - t), wb = (1.f - eps) * t, u = eps / (float)C;   // (xent_mix_kernel's)
  const float qnan = __builtin_nanf("");
  const float invB = 1.0f / B;
  const float gsc = invB * dscale * (loss_scale ? *loss_scale : 1.f);
  const float oma = 1.f - alpha;
  const float la = lr[ya];
  float dot = (1.f - eps) * (la + t * (lr[yb] - la));
  if (u != 0.f) dot += u * sl;
  if (HARD) {
    float bx = -INFINITY;
    int bc = C;   // (-inf at index C loses against every class of a finite row)
    for (int c = lane; c < C; c += 64)
      if (tr[c] > bx) {
        bx = tr[c];
        bc = c;
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ox = __shfl_xor(bx, o, 64);
      const int oc = __shfl_xor(bc, o, 64);
      if (ox > bx || (ox == bx && oc < bc)) {
        bx = ox;
        bc = oc;
      }
    }
    const int yt = ok ? bc : 0;
    if (dlogits)
      for (int c = lane; c < C; c += 64) {
        const float q = (c == ya ? wa : 0.f) + (c == yb ? wb : 0.f) + u;
        const float qd = oma * q + (c == yt ? alpha : 0.f);
        dlogits[(size_t)b * C + c] = ok ? (__expf(lr[c] - lse) - qd) * gsc : qnan;
      }
    if (lane == 0) loss_per[b] = ok ? (lse - (oma * dot + alpha * lr[yt])) * invB : qnan;
  } else {
    const float invT = 1.f / T, aT = alpha * T, aT2 = aT * T;
    const float lseZ = tempered_lse(lr, C, lane, invT), lseT = tempered_lse(tr, C, lane, invT);
    float kl = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float lz = lr[c] * invT - lseZ, lt = tr[c] * invT - lseT;
      const float pT = __expf(lz), r = __expf(lt);
      kl += r * (lt - lz);
      if (dlogits) {
        const float q = (c == ya ? wa : 0.f) + (c == yb ? wb : 0.f) + u;
        dlogits[(size_t)b * C + c] = ok ? (oma * (__expf(lr[c] - lse) - q) + aT * (pT - r)) * gsc : qnan;
      }
    }
    kl = wave_sum(kl);
    if (lane == 0) loss_per[b] = ok ? (oma * (lse - dot) + aT2 * kl) * invB : qnan;
  }
}
__global__ __launch_bounds__(64) void xent_sum_kernel(const float* __restrict__ loss_per, float* __restrict__ loss, int B,
                                                      float* __restrict__ found_inf) {
  float s = 0.f;
  for (int b = threadIdx.x; b < B; b += 64) s += loss_per[b];
  s = wave_sum(s);
  if (threadIdx.x == 0) {
    *loss = s;
    if (found_inf) *found_inf = 0.f;   // raised by the backward's final gradient writes (cara_vit_shape::found_inf)
  }
}

__global__ __launch_bounds__(256) void cvt_kernel(const float* __restrict__ src, bf16* __restrict__ dst, size_t n) {
  const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i + 3 < n) {
    const float4 v = *reinterpret_cast<const float4*>(src + i);
    bf16x4 o = {(bf16)v.x, (bf16)v.y, (bf16)v.z, (bf16)v.w};
    *reinterpret_cast<bf16x4*>(dst + i) = o;
  } else {
    for (size_t k = i; k < n; ++k) dst[k] = (bf16)src[k];
  }
}

// dst[c][r] = src[r][c], 32x32 tiles through LDS
__global__ __launch_bounds__(256) void transpose_kernel(const bf16* __restrict__ src, bf16* __restrict__ dst,
                                                        int rows, int cols) {
  __shared__ bf16 tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  for (int k = ty; k < 32; k += 8)
    if (r0 + k < rows && c0 + tx < cols) tile[k][tx] = src[(size_t)(r0 + k) * cols + c0 + tx];
  __syncthreads();
  for (int k = ty; k < 32; k += 8)
    if (c0 + k < cols && r0 + tx < rows) dst[(size_t)(c0 + k) * rows + r0 + tx] = tile[tx][k];
}

// dst[c * ldd + r] = src[r * lds + c] for a [rows, cols] matrix, 64 x 64 tiles, 16-byte global accesses both ways
// (activation-sized transposes of the exact weight-dropout mode: dY^T and X^T feed the dense dW GEMM)
__global__ __launch_bounds__(256) void transpose64_kernel(const bf16* __restrict__ src, long lds_, bf16* __restrict__ dst, long ldd,
                                                          int rows, int cols) {
  __shared__ bf16 tile[64][72];
  const int t = threadIdx.x, c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = (t >> 3) + 32 * j, c = (t & 7) * 8;
    bf16x8 v = {};
    if (r0 + r < rows) {
      if (c0 + c + 8 <= cols) {
        v = *reinterpret_cast<const bf16x8*>(src + (size_t)(r0 + r) * lds_ + c0 + c);
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (c0 + c + k < cols) v[k] = src[(size_t)(r0 + r) * lds_ + c0 + c + k];
      }
    }
    *reinterpret_cast<bf16x8*>(&tile[r][c]) = v;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = (t >> 3) + 32 * j, r = (t & 7) * 8;   // output row c0 + c, 8 consecutive source rows
    if (c0 + c >= cols) continue;
    bf16x8 v;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = tile[r + k][c];
    bf16* d = dst + (size_t)(c0 + c) * ldd + r0 + r;
    if (r0 + r + 8 <= rows) {
      *reinterpret_cast<bf16x8*>(d) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (r0 + r + k < rows) d[k] = v[k];
    }
  }
}

}  // namespace

namespace {
struct XuArgs {   // optional fused skinny product (all NULL / 0 = plain LayerNorm)
  const bf16* Ut;
  int rank, Rp;
  bf16 *T, *Tt;
  int ldt;
};
bool xu_ok(const XuArgs& a, int M, int C) {
  if (!a.Ut) return true;
  // Rp / 16 column tiles of 16 (rows of Ut beyond the rank are zero, so the pad columns come out zero)
  return a.T && (a.Rp == 32 || a.Rp == 64) && a.rank > 0 && a.rank <= a.Rp && (!a.Tt || (a.ldt >= M && !(a.ldt & 7))) &&
         cara_layernorm_takes(C, true);
}
// consumers (cara_tskinny_*) read Tt in whole 32-row steps: keep columns [M, roundup32(M)) zero (as cara_skinny_xu does)
int xu_pad(const XuArgs& a, int M, hipStream_t st) {
  const int m32 = (M + 31) / 32 * 32;
  if (a.Ut && a.Tt && m32 > M && m32 <= a.ldt &&
      hipMemset2DAsync(a.Tt + M, (size_t)a.ldt * 2, 0, (size_t)(m32 - M) * 2, a.Rp, st) != hipSuccess)
    return CARA_E_LAUNCH;
  return CARA_OK;
}

// (C, fused contraction?, its column tiles) -> the template arguments <V4, XU, NT> of ln_fwd_kernel / ln_bwd_kernel, handed to
// `launch` as integral constants.  Column tiles of the contraction: Rp / 16, or one where half of the padded rank is structurally
// zero (Rp = 32, rank <= 16).  false: a C the kernels do not take.
template <int N> using Int = std::integral_constant<int, N>;
template <class Launch>
bool ln_dispatch(int C, const XuArgs& a, Launch&& launch) {
  if (!cara_layernorm_takes(C, a.Ut != nullptr)) return false;
  auto with_dim = [&](auto xu, auto nt) {
    if (C == 768) launch(Int<3>{}, xu, nt);
    else if (C == 1024) launch(Int<4>{}, xu, nt);
    else launch(Int<1>{}, xu, nt);
  };
  if (a.Ut && a.Rp == 64) with_dim(std::true_type{}, Int<4>{});
  else if (a.Ut && a.rank <= 16) with_dim(std::true_type{}, Int<1>{});
  else if (a.Ut) with_dim(std::true_type{}, Int<2>{});
  else with_dim(std::false_type{}, Int<2>{});
  return true;
}

int ln_fwd_launch(const float* x, long ldx, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int M,
                  int C, float eps, const XuArgs& a, void* stream, int yp = 0) {
  if (!x || !gamma || !beta || !y || !mean || !rstd || M <= 0 || ldx < C || (ldx & 3) || !xu_ok(a, M, C)) return CARA_E_ARG;
  if (yp && yp < M) return CARA_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (xu_pad(a, M, st) != CARA_OK) return CARA_E_LAUNCH;
  const int rows_per_block = a.Ut ? 16 : 4;
  const dim3 grid((M + rows_per_block - 1) / rows_per_block), block(a.Ut ? XU_WAVES * 64 : 256);
  if (!ln_dispatch(C, a, [&](auto v, auto xu, auto nt) {
        hipLaunchKernelGGL((ln_fwd_kernel<decltype(v)::value, decltype(xu)::value, decltype(nt)::value>), grid, block, 0, st, x, ldx, gamma, beta, (bf16*)y, mean, rstd, M, eps,
                           a.Ut, a.rank, a.Rp, a.T, a.Tt, a.ldt, yp);
      }))
    return CARA_E_ARG;
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}

int ln_bwd_launch(const void* dy, const float* x, long ldx, const float* gamma, const float* mean, const float* rstd,
                  const float* dx_in, float* dx_out, void* dyb, const float* rowscale, int rows_per_sample, int M, int C,
                  const XuArgs& a, void* stream, int yp = 0, int dx_in_every = 0) {
  if (!dy || !x || !gamma || !mean || !rstd || !dx_out || M <= 0 || ldx < C || (ldx & 3) || !xu_ok(a, M, C)) return CARA_E_ARG;
  if (yp && (yp < M || !dyb)) return CARA_E_ARG;
  if (rowscale && rows_per_sample <= 0) return CARA_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (xu_pad(a, M, st) != CARA_OK) return CARA_E_LAUNCH;
  const int rows_per_block = a.Ut ? 16 : 4;
  const dim3 grid((M + rows_per_block - 1) / rows_per_block), block(a.Ut ? XU_WAVES * 64 : 256);
  if (!ln_dispatch(C, a, [&](auto v, auto xu, auto nt) {
        hipLaunchKernelGGL((ln_bwd_kernel<decltype(v)::value, decltype(xu)::value, decltype(nt)::value>), grid, block, 0, st, (const bf16*)dy, x, ldx, gamma, mean, rstd, dx_in,
                           dx_out, (bf16*)dyb, rowscale, rows_per_sample, M, a.Ut, a.rank, a.Rp, a.T, a.Tt, a.ldt, yp, dx_in_every);
      }))
    return CARA_E_ARG;
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}
}  // namespace

// The row lengths ln_fwd_kernel / ln_bwd_kernel are instantiated for (V4 = C / 256 float4 per lane), with and without the fused
// contraction: today the same three (declared in common.h: vit.hip's plan asks before it fuses)
bool cara_layernorm_takes(int C, bool /* fused */) {
  return C == 768 || C == 1024 || C == 256;
}

extern "C" int cara_layernorm_fwd(const float* x, long ldx, const float* gamma, const float* beta, void* y,
                                  float* mean, float* rstd, int M, int C, float eps, void* stream) {
  return ln_fwd_launch(x, ldx, gamma, beta, y, mean, rstd, M, C, eps, XuArgs{nullptr, 0, 0, nullptr, nullptr, 0}, stream);
}
extern "C" int cara_layernorm_fwd_xu(const float* x, long ldx, const float* gamma, const float* beta, void* y,
                                     float* mean, float* rstd, int M, int C, float eps, const void* Ut, int rank, int Rp,
                                     void* T, void* Tt, int ldt, void* stream) {
  if (!Ut) return CARA_E_ARG;
  return ln_fwd_launch(x, ldx, gamma, beta, y, mean, rstd, M, C, eps,
                       XuArgs{static_cast<const bf16*>(Ut), rank, Rp, static_cast<bf16*>(T), static_cast<bf16*>(Tt), ldt}, stream);
}
extern "C" int cara_layernorm_bwd(const void* dy, const float* x, long ldx, const float* gamma, const float* mean,
                                  const float* rstd, const float* dx_in, float* dx_out, void* dyb,
                                  const float* rowscale, int rows_per_sample, int M, int C, void* stream) {
  return ln_bwd_launch(dy, x, ldx, gamma, mean, rstd, dx_in, dx_out, dyb, rowscale, rows_per_sample, M, C,
                       XuArgs{nullptr, 0, 0, nullptr, nullptr, 0}, stream);
}
extern "C" int cara_layernorm_bwd_xu(const void* dy, const float* x, long ldx, const float* gamma, const float* mean,
                                     const float* rstd, const float* dx_in, float* dx_out, void* dyb,
                                     const float* rowscale, int rows_per_sample, int M, int C, const void* Vst, int rank,
                                     int Rp, void* G, void* Gt, int ldt, void* stream) {
  if (!Vst) return CARA_E_ARG;
  return ln_bwd_launch(dy, x, ldx, gamma, mean, rstd, dx_in, dx_out, dyb, rowscale, rows_per_sample, M, C,
                       XuArgs{static_cast<const bf16*>(Vst), rank, Rp, static_cast<bf16*>(G), static_cast<bf16*>(Gt), ldt}, stream);
}
// The general forms: Ut may be NULL (no fused contraction), and the bf16 output (y, resp. dyb) can be written
// K-panel-major -- [C/32][panels][32], panels >= M rows per panel -- the layout cara_gemm_args::a_panels reads.
extern "C" int cara_layernorm_fwd_ex(const float* x, long ldx, const float* gamma, const float* beta, void* y,
                                     float* mean, float* rstd, int M, int C, float eps, const void* Ut, int rank, int Rp,
                                     void* T, void* Tt, int ldt, int y_panels, void* stream) {
  if (y_panels < 0) return CARA_E_ARG;
  const XuArgs a = Ut ? XuArgs{static_cast<const bf16*>(Ut), rank, Rp, static_cast<bf16*>(T), static_cast<bf16*>(Tt), ldt}
                      : XuArgs{nullptr, 0, 0, nullptr, nullptr, 0};
  return ln_fwd_launch(x, ldx, gamma, beta, y, mean, rstd, M, C, eps, a, stream, y_panels);
}
extern "C" int cara_layernorm_bwd_ex(const void* dy, const float* x, long ldx, const float* gamma, const float* mean,
                                     const float* rstd, const float* dx_in, float* dx_out, void* dyb, const float* rowscale,
                                     int rows_per_sample, int M, int C, const void* Vst, int rank, int Rp, void* G, void* Gt,
                                     int ldt, int dyb_panels, void* stream) {
  if (dyb_panels < 0) return CARA_E_ARG;
  const XuArgs a = Vst ? XuArgs{static_cast<const bf16*>(Vst), rank, Rp, static_cast<bf16*>(G), static_cast<bf16*>(Gt), ldt}
                       : XuArgs{nullptr, 0, 0, nullptr, nullptr, 0};
  return ln_bwd_launch(dy, x, ldx, gamma, mean, rstd, dx_in, dx_out, dyb, rowscale, rows_per_sample, M, C, a, stream, dyb_panels);
}

// cara_layernorm_bwd_ex with dx_in read on every dx_in_every-th row only (not in include/cara_hip.h: vit.hip's last block)
int cara_layernorm_bwd_rows_in(const void* dy, const float* x, long ldx, const float* gamma, const float* mean, const float* rstd,
                               const float* dx_in, float* dx_out, void* dyb, const float* rowscale, int rows_per_sample, int M, int C,
                               const void* Vst, int rank, int Rp, void* G, void* Gt, int ldt, int dyb_panels, int dx_in_every,
                               void* stream) {
  if (dyb_panels < 0 || dx_in_every < 0) return CARA_E_ARG;
  const XuArgs a = Vst ? XuArgs{static_cast<const bf16*>(Vst), rank, Rp, static_cast<bf16*>(G), static_cast<bf16*>(Gt), ldt}
                       : XuArgs{nullptr, 0, 0, nullptr, nullptr, 0};
  return ln_bwd_launch(dy, x, ldx, gamma, mean, rstd, dx_in, dx_out, dyb, rowscale, rows_per_sample, M, C, a, stream, dyb_panels, dx_in_every);
}

extern "C" int cara_assemble_tokens(const float* emb, const float* cls, const float* pos, float* x, int B, int P,
                                    int D, void* stream) {
  if (!emb || !cls || !pos || !x || B <= 0 || P <= 0 || D <= 0 || (D & 3)) return CARA_E_ARG;
  const long total4 = (long)B * (P + 1) * D / 4;
  hipLaunchKernelGGL(assemble_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     emb, cls, pos, x, B, P, D, total4);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}

extern "C" int cara_assemble_tokens_keep(const float* emb, const float* cls, const float* pos, const int* keep, float* x, int B, int K,
                                         int P, int D, void* stream) {
  if (!emb || !cls || !pos || !keep || !x || B <= 0 || K <= 0 || K > P || D <= 0 || (D & 3)) return CARA_E_ARG;
  const long total4 = (long)B * (K + 1) * D / 4;
  hipLaunchKernelGGL(assemble_keep_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     emb, cls, pos, keep, x, B, K, P, D, total4);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}

extern "C" int cara_cross_entropy_ex(const float* logits, const int64_t* labels, float* loss, float* dlogits, int B,
                                     int C, float dscale, const float* loss_scale, float* found_inf, void* stream) {
  // loss doubles as scratch: needs room for 1 + B floats (loss[0] = mean loss, loss[1..B] per-sample terms)
  if (!logits || !labels || !loss || B <= 0 || C <= 0 || !(dscale > 0.f)) return CARA_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(xent_kernel, dim3(B), dim3(64), 0, st, logits, labels, loss + 1, dlogits, B, C, dscale, loss_scale);
  CARA_CHECK_LAUNCH();
  hipLaunchKernelGGL(xent_sum_kernel, dim3(1), dim3(64), 0, st, loss + 1, loss, B, found_inf);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}
extern "C" int cara_cross_entropy_mix(const float* logits, const int64_t* labels, const int* mix, float smoothing, float* loss,
                                      float* dlogits, int B, int C, float dscale, const float* loss_scale, float* found_inf,
                                      void* stream) {
  if (!logits || !labels || !loss || B <= 0 || C <= 0 || !(dscale > 0.f) || !(smoothing >= 0.f && smoothing < 1.f)) return CARA_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(xent_mix_kernel, dim3(B), dim3(64), 0, st, logits, labels, mix, smoothing, loss + 1, dlogits, B, C, dscale, loss_scale);
  CARA_CHECK_LAUNCH();
  hipLaunchKernelGGL(xent_sum_kernel, dim3(1), dim3(64), 0, st, loss + 1, loss, B, found_inf);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}
extern "C" int cara_cross_entropy_bal(const float* logits, const int64_t* labels, const int* mix, float smoothing,
                                      const float* class_weight, const float* logit_bias, float* loss, float* dlogits, int B, int C,
                                      float dscale, const float* loss_scale, float* found_inf, void* stream) {
  // (without a weight and a bias this IS cara_cross_entropy_mix: the same launches, bit for bit)
  if (!class_weight && !logit_bias)
    return cara_cross_entropy_mix(logits, labels, mix, smoothing, loss, dlogits, B, C, dscale, loss_scale, found_inf, stream);
  if (!logits || !labels || !loss || B <= 0 || C <= 0 || !(dscale > 0.f) || !(smoothing >= 0.f && smoothing < 1.f)) return CARA_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(xent_bal_kernel, dim3(B), dim3(64), 0, st, logits, labels, mix, smoothing, class_weight, logit_bias, loss + 1,
                     dlogits, B, C, dscale, loss_scale);
  CARA_CHECK_LAUNCH();
  hipLaunchKernelGGL(xent_sum_kernel, dim3(1), dim3(64), 0, st, loss + 1, loss, B, found_inf);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}
extern "C" int cara_sigmoid_loss(const float* logits, const int64_t* labels, const int* mix, float smoothing, float target_threshold,
                                 float gamma, float alpha, const float* pos_weight, int sum_classes, float* loss, float* dlogits,
                                 int B, int C, float dscale, const float* loss_scale, float* found_inf, void* stream) {
  if (!logits || !labels || !loss || B <= 0 || C <= 0 || !(dscale > 0.f) || !(smoothing >= 0.f && smoothing < 1.f)) return CARA_E_ARG;
  // (every comparison is written so that a NaN fails it)
  if (!(target_threshold < 1.f) || !(alpha <= 1.f) || (sum_classes != 0 && sum_classes != 1)) return CARA_E_ARG;
  if (!(gamma == 0.f || (gamma >= 1.f && gamma <= 3.0e38f))) return CARA_E_ARG;
  const bool focal = gamma > 0.f || alpha >= 0.f;
  if (focal && pos_weight) return CARA_E_ARG;
  const float thr = target_threshold < 0.f ? -1.f : target_threshold, al = alpha < 0.f ? -1.f : alpha;
  const float invBD = (float)(1.0 / ((double)B * (double)(sum_classes ? 1 : C)));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (focal)
    hipLaunchKernelGGL(sigmoid_loss_kernel<true>, dim3(B), dim3(64), 0, st, logits, labels, mix, smoothing, thr, gamma, al, nullptr,
                       loss + 1, dlogits, B, C, invBD, dscale, loss_scale);
  else
    hipLaunchKernelGGL(sigmoid_loss_kernel<false>, dim3(B), dim3(64), 0, st, logits, labels, mix, smoothing, thr, 0.f, -1.f, pos_weight,
                       loss + 1, dlogits, B, C, invBD, dscale, loss_scale);
  CARA_CHECK_LAUNCH();
  hipLaunchKernelGGL(xent_sum_kernel, dim3(1), dim3(64), 0, st, loss + 1, loss, B, found_inf);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}
extern "C" int cara_distill_loss(const float* logits, const float* teacher, const int64_t* labels, const int* mix, float smoothing,
                                 float alpha, float temperature, int hard, float* loss, float* dlogits, int B, int C, float dscale,
                                 const float* loss_scale, float* found_inf, void* stream) {
  // (every comparison is written so that a NaN fails it)
  if (!(alpha >= 0.f && alpha <= 1.f) || (hard != 0 && hard != 1)) return CARA_E_ARG;
  // (without a teacher's share this IS cara_cross_entropy_mix: the same launches, bit for bit; the teacher is not read)
  if (alpha == 0.f) return cara_cross_entropy_mix(logits, labels, mix, smoothing, loss, dlogits, B, C, dscale, loss_scale, found_inf, stream);
  if (!logits || !labels || !loss || B <= 0 || C <= 0 || !(dscale > 0.f) || !(smoothing >= 0.f && smoothing < 1.f)) return CARA_E_ARG;
  // (a temperature so small that the fp32 1 / T is infinite would turn every tempered logit into inf or NaN: refused like T <= 0)
  if (!teacher || (!hard && !(temperature > 0.f && temperature <= 3.4028235e38f && 1.f / temperature <= 3.4028235e38f))) return CARA_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hard)
    hipLaunchKernelGGL(distill_kernel<true>, dim3(B), dim3(64), 0, st, logits, teacher, labels, mix, smoothing, alpha, 1.f, loss + 1, dlogits,
                       B, C, dscale, loss_scale);
  else
    hipLaunchKernelGGL(distill_kernel<false>, dim3(B), dim3(64), 0, st, logits, teacher, labels, mix, smoothing, alpha, temperature, loss + 1,
                       dlogits, B, C, dscale, loss_scale);
  CARA_CHECK_LAUNCH();
  hipLaunchKernelGGL(xent_sum_kernel, dim3(1), dim3(64), 0, st, loss + 1, loss, B, found_inf);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}
extern "C" int cara_cross_entropy(const float* logits, const int64_t* labels, float* loss, float* dlogits, int B,
                                  int C, void* stream) {
  return cara_cross_entropy_ex(logits, labels, loss, dlogits, B, C, 1.f, nullptr, nullptr, stream);
}

extern "C" int cara_f32_to_bf16(const float* src, void* dst, size_t n, void* stream) {
  if (!src || !dst || n == 0) return CARA_E_ARG;
  const size_t nthreads = (n + 3) / 4;
  hipLaunchKernelGGL(cvt_kernel, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     src, (bf16*)dst, n);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}

extern "C" int cara_transpose_bf16_ld(const void* src, long lds, void* dst, long ldd, int rows, int cols, void* stream) {
  if (!src || !dst || rows <= 0 || cols <= 0 || lds < cols || ldd < rows || (lds & 7) || (ldd & 7)) return CARA_E_ARG;
  hipLaunchKernelGGL(transpose64_kernel, dim3((cols + 63) / 64, (rows + 63) / 64), dim3(256), 0, static_cast<hipStream_t>(stream),
                     (const bf16*)src, lds, (bf16*)dst, ldd, rows, cols);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}

extern "C" int cara_transpose_bf16(const void* src, void* dst, int rows, int cols, void* stream) {
  if (!src || !dst || rows <= 0 || cols <= 0) return CARA_E_ARG;
  hipLaunchKernelGGL(transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0,
                     static_cast<hipStream_t>(stream), (const bf16*)src, (bf16*)dst, rows, cols);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}
