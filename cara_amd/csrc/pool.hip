// Mean-pooled readout (timm's global_pool = "avg" with fc_norm): the mean of a sample's patch tokens and its backward (gfx950).
// Both kernels are HBM-bound passes over one [B, tokens, D] fp32 tensor; neither uses atomics, so the same input gives the same bits.
#include "common.h"

namespace {

// A workgroup owns POOL_COLS float4 columns (512 contiguous bytes of every row) of one sample; its POOL_GROUPS token groups take the
// tokens first + g, first + g + POOL_GROUPS, ... each.  At B = 64, D = 768 that is 6 x 64 = 384 workgroups for 256 CUs.
constexpr int POOL_COLS = 32;
constexpr int POOL_GROUPS = 8;

// out[b, :] = (sum over t in [first, tokens) of x[b, t, :]) / n.  The order is fixed: every group adds its tokens in ascending order
// starting FROM its first token (not from zero), then the groups that have a token are added in ascending order -- with one token
// the row goes through untouched, bit for bit.  Rows below `first` are never read.
__global__ __launch_bounds__(POOL_COLS * POOL_GROUPS) void token_mean_kernel(const float* __restrict__ x, int tokens, int first, int D4,
                                                                              float* __restrict__ out) {
  __shared__ float4 part[POOL_GROUPS][POOL_COLS];
  const int c = threadIdx.x % POOL_COLS, g = threadIdx.x / POOL_COLS;
  const int col = blockIdx.x * POOL_COLS + c, b = blockIdx.y;
  const int n = tokens - first;
  if (col < D4 && g < n) {
    const float4* xr = reinterpret_cast<const float4*>(x) + ((size_t)b * tokens + first) * D4 + col;
    float4 s = xr[(size_t)g * D4];
#pragma unroll 8
    for (int t = g + POOL_GROUPS; t < n; t += POOL_GROUPS) {
      const float4 v = xr[(size_t)t * D4];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    part[g][c] = s;
  }
  __syncthreads();
  if (g == 0 && col < D4) {
    const int ng = n < POOL_GROUPS ? n : POOL_GROUPS;
    float4 s = part[0][c];
    for (int k = 1; k < ng; ++k) {
      const float4 v = part[k][c];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    const float fn = (float)n;   // (a correctly rounded division: one rounding behind the sum, exact at n = 1)
    reinterpret_cast<float4*>(out)[(size_t)b * D4 + col] = make_float4(s.x / fn, s.y / fn, s.z / fn, s.w / fn);
  }
}

// dx[b, t, :] = dpool[b, :] / n for t >= first, 0 below; dyb = the 16-bit image of rowscale[b] * dx, row-major or K-panel-major
// ([D/32][panels][32], as ln_bwd_kernel writes it).  A workgroup: POOL_COLS float4 columns of POOL_ROWS token rows of one sample.
constexpr int POOL_ROWS = 64;
__global__ __launch_bounds__(POOL_COLS * POOL_GROUPS) void token_mean_bwd_kernel(const float* __restrict__ dpool,
                                                                                  const float* __restrict__ rowscale, int tokens,
                                                                                  int first, int D4, float* __restrict__ dx,
                                                                                  bf16* __restrict__ dyb, int panels) {
  const int c = threadIdx.x % POOL_COLS, g = threadIdx.x / POOL_COLS;
  const int col = blockIdx.x * POOL_COLS + c, b = blockIdx.y;
  if (col >= D4) return;
  const float fn = (float)(tokens - first);
  const float4 d = reinterpret_cast<const float4*>(dpool)[(size_t)b * D4 + col];
  const float4 v = make_float4(d.x / fn, d.y / fn, d.z / fn, d.w / fn);
  const float sc = rowscale ? rowscale[b] : 1.f;
  float4 vs = make_float4(v.x * sc, v.y * sc, v.z * sc, v.w * sc);
  // (the product is an fp32 value in both builds before it is rounded to 16 bits, as in ln_bwd_kernel)
  asm volatile("" : "+v"(vs.x), "+v"(vs.y), "+v"(vs.z), "+v"(vs.w));
  const bf16x4 h = {(bf16)vs.x, (bf16)vs.y, (bf16)vs.z, (bf16)vs.w};
  const bf16x4 hz = {(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const int t1 = (blockIdx.z + 1) * POOL_ROWS < tokens ? (blockIdx.z + 1) * POOL_ROWS : tokens;
  const int c0 = col * 4;
  for (int t = blockIdx.z * POOL_ROWS + g; t < t1; t += POOL_GROUPS) {
    const size_t row = (size_t)b * tokens + t;
    const bool live = t >= first;
    reinterpret_cast<float4*>(dx)[row * D4 + col] = live ? v : z;
    bf16* p = panels ? dyb + ((size_t)(c0 >> 5) * panels + row) * 32 + (c0 & 31) : dyb + row * D4 * 4 + c0;
    *reinterpret_cast<bf16x4*>(p) = live ? h : hz;
  }
}

}  // namespace

extern "C" int cara_token_mean(const float* x, int B, int tokens, int first, int D, float* out, void* stream) {
  if (!x || !out || B <= 0 || first < 0 || tokens <= first || D <= 0 || (D & 3)) return CARA_E_ARG;
  if (B > 65535 || (long long)B * tokens >= (1ll << 31)) return CARA_E_ARG;
  const int D4 = D / 4;
  hipLaunchKernelGGL(token_mean_kernel, dim3((D4 + POOL_COLS - 1) / POOL_COLS, B), dim3(POOL_COLS * POOL_GROUPS), 0,
                     static_cast<hipStream_t>(stream), x, tokens, first, D4, out);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}

extern "C" int cara_token_mean_bwd(const float* dpool, const float* rowscale, int B, int tokens, int first, int D, float* dx, void* dyb,
                                   int dyb_panels, void* stream) {
  if (!dpool || !dx || !dyb || B <= 0 || first < 0 || tokens <= first || D <= 0 || (D & 3)) return CARA_E_ARG;
  if (B > 65535 || (long long)B * tokens >= (1ll << 31)) return CARA_E_ARG;
  // K-panel-major: whole panels of 32 columns, every row inside a panel
  if (dyb_panels < 0 || (dyb_panels > 0 && ((D & 31) || (long long)dyb_panels < (long long)B * tokens))) return CARA_E_ARG;
  const int D4 = D / 4, zt = (tokens + POOL_ROWS - 1) / POOL_ROWS;
  if (zt > 65535) return CARA_E_ARG;
  hipLaunchKernelGGL(token_mean_bwd_kernel, dim3((D4 + POOL_COLS - 1) / POOL_COLS, B, zt), dim3(POOL_COLS * POOL_GROUPS), 0,
                     static_cast<hipStream_t>(stream), dpool, rowscale, tokens, first, D4, dx, static_cast<bf16*>(dyb), dyb_panels);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}
