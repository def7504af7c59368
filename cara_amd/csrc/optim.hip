// AdamW over the trainable tensors of a step (12 CP tensors + the classifier head: ~1.2e5 elements at rank 16) as ONE launch.
// The reference steps torch.optim.AdamW (image_classification/vit_cp.py:185, :50); its fused CUDA/HIP path spends 42 us per step
// on these few small tensors (rocprofv3: multi_tensor_apply_kernel, 20 workgroups), a kernel of our own 3-4 us.
//
// Arithmetic = torch.optim.AdamW (amsgrad = False, maximize = False), element by element in fp32:
//   p   *= 1 - lr * weight_decay                         (decoupled decay)
//   m    = m + (1 - beta1) (g - m)                        (exp_avg.lerp_)
//   v    = beta2 v + (1 - beta2) g g
//   p   -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
// The tensors come BY VALUE in the kernel arguments (pointers and sizes of up to 32 tensors, 1.3 KiB): no table in device
// memory, nothing to upload when a learning rate changes.
// Beside it: the loss-scale update of the IEEE-half build, and gradient accumulation and global-norm clipping over the step's one
// flat gradient buffer (cara_grad_accumulate, cara_grad_clip), and the moving average of the trainable tensors, AdamW's scheme again
// (cara_ema_update), and the two launches of sharpness-aware minimisation around a step's second pass (cara_sam_perturb,
// cara_sam_restore).
#include "common.h"

namespace {

constexpr int ADAMW_CHUNK = 1024;   // elements per workgroup (256 threads x 4)

__global__ __launch_bounds__(256) void adamw_kernel(const cara_adamw_args a) {
  // which tensor this workgroup works on: a prefix walk over <= 32 entries (uniform)
  int t = 0, first = 0;
  for (; t < a.ntensors; ++t) {
    const int nchunk = (int)((a.t[t].n + ADAMW_CHUNK - 1) / ADAMW_CHUNK);
    if ((int)blockIdx.x < first + nchunk) break;
    first += nchunk;
  }
  if (t >= a.ntensors) return;
  if (a.skip_flag && *a.skip_flag != 0.f) return;   // the step's gradients overflowed under the loss scale: nothing moves
  const cara_adamw_tensor& T = a.t[t];
  float lr = a.lr[T.group], bc1 = a.bias_correction1, bc2s = a.bias_correction2_sqrt;
  if (a.dyn) {   // the capturable form: step count and learning rates live in device memory (cara_adamw_args::dyn)
    const float tt = a.dyn[0];
    lr = a.dyn[1 + T.group];
    bc1 = 1.f - powf(1.f - a.one_minus_beta1, tt);
    bc2s = sqrtf(1.f - powf(a.beta2, tt));
  }
  const float wd = a.weight_decay[T.group];
  const float decay = 1.f - lr * wd;
  const float step_size = lr / bc1;
  float* __restrict__ p = T.p;
  const float* __restrict__ g = T.g;
  float* __restrict__ m = T.m;
  float* __restrict__ v = T.v;
  const size_t base = (size_t)((int)blockIdx.x - first) * ADAMW_CHUNK;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const size_t i = base + (size_t)j * 256 + threadIdx.x;
    if (i >= T.n) continue;
    const float gi = g[i];
    float pi = p[i] * decay;
    const float mi = m[i] + a.one_minus_beta1 * (gi - m[i]);
    const float vi = a.beta2 * v[i] + a.one_minus_beta2 * gi * gi;
    const float denom = sqrtf(vi) / bc2s + a.eps;
    pi -= step_size * (mi / denom);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
  }
}

// GradScaler's update rule on the device: one thread (cara_hip.h, cara_amp_update)
__global__ void amp_update_kernel(float* __restrict__ st, const float* __restrict__ found_inf, float growth, float backoff,
                                  int interval, float max_scale) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (*found_inf != 0.f) {
    st[0] = fmaxf(st[0] * backoff, 1.f);
    st[1] = 0.f;
    st[2] += 1.f;
  } else {
    const float n = st[1] + 1.f;
    if (n >= (float)interval) {
      st[0] = fminf(st[0] * growth, max_scale);
      st[1] = 0.f;
    } else {
      st[1] = n;
    }
  }
}

// ---- gradient accumulation and global-norm clipping over ONE flat fp32 buffer (cara_hip.h: cara_grad_accumulate, cara_grad_clip) ----
// Both are latency-bound launches over 0.5 MB (rank 16) to some tens of MB: 16-byte accesses, few resident workgroups, no atomics.

// dst = a + b (b == NULL: dst = a), one fp32 rounding per element.  Elements [head, head + 4 nvec) go as float4 (the host passes
// nvec > 0 only when all pointers share dst's residue mod 16), the rest -- at most 3 + 3 elements then, everything otherwise -- one by
// one.  An element is read and written by the same thread, so dst may be a or b.
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* dst, const float* a, const float* b, size_t n, size_t head,
                                                              size_t nvec) {
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  for (size_t v = tid; v < nvec; v += stride) {
    const size_t i = head + 4 * v;
    f32x4 x = *reinterpret_cast<const f32x4*>(a + i);
    if (b) {
      const f32x4 y = *reinterpret_cast<const f32x4*>(b + i);
      x += y;
    }
    *reinterpret_cast<f32x4*>(dst + i) = x;
  }
  const size_t body_end = head + 4 * nvec, nedge = head + (n - body_end);
  for (size_t e = tid; e < nedge; e += stride) {
    const size_t i = e < head ? e : body_end + (e - head);
    dst[i] = b ? a[i] + b[i] : a[i];
  }
}

// THE REDUCTION TREE of cara_grad_clip (tests/optim_model.py restates it and derives the test bound from it).
// A chunk is CLIP_CHUNK = 8192 consecutive elements; 256 threads (4 waves) per workgroup.
//   1. thread t: acc = 0; for j = 0 .. 7, for c = 0 .. 3: acc = acc + g[8192 chunk + 4 (256 j + t) + c]^2  (elements past n add 0):
//      one rounding per square, 32 sequential additions (the first one, to 0, is exact: 31);
//   2. the wave's 64 accumulators: the butterfly of wave_sum, lanes 32, 16, 8, 4, 2, 1 apart: 6 additions;
//   3. the four wave sums, left to right ((w0 + w1) + w2) + w3: 3 additions                      -> partial[chunk]   (launch 1)
//   4. thread t of EVERY workgroup of launch 2: acc = 0; for q = t, t + 256, ... < chunks: acc = acc + partial[q]
//      (ceil(chunks / 256) sequential additions), then steps 2 and 3 again: 6 + 3 additions      -> total, the same bits everywhere
// Longest path: 31 + 6 + 3 + ceil(chunks / 256) + 6 + 3 additions, one rounding per square before them, one sqrtf after.
// Every product and sum is a single IEEE operation: these kernels are written with plain operators under `fp contract(off)` (hipcc's
// default fuses acc + x * x into an fma, through __fmul_rn / __fadd_rn too, and the square would lose its own rounding).
constexpr int CLIP_CHUNK = 8192;
constexpr int CLIP_MAX_GRID = 2048;   // launch 2 walks the chunks grid-strided above this many (n > 16.7 M elements)

__device__ __forceinline__ float clip_block_sum(float acc, float* lds) {
#pragma clang fp contract(off)
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
  __syncthreads();
  const float s = ((lds[0] + lds[1]) + lds[2]) + lds[3];
  __syncthreads();
  return s;
}

template <bool VEC>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* g, size_t n, float* partial) {
#pragma clang fp contract(off)
  __shared__ float lds[4];
  const size_t base = (size_t)blockIdx.x * CLIP_CHUNK;
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const size_t i = base + 4 * ((size_t)j * 256 + threadIdx.x);
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    if (VEC && i + 4 <= n) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(g + i);
      x[0] = v[0]; x[1] = v[1]; x[2] = v[2]; x[3] = v[3];
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (i + c < n) x[c] = g[i + c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float sq = x[c] * x[c];
      acc = acc + sq;
    }
  }
  const float s = clip_block_sum(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

template <bool VEC>
__global__ __launch_bounds__(256) void grad_scale_kernel(float* g, size_t n, size_t chunks, float max_norm, const float* partial,
                                                         const float* found_inf, float* out) {
#pragma clang fp contract(off)
  __shared__ float lds[4];
  float acc = 0.f;
  for (size_t q = threadIdx.x; q < chunks; q += 256) acc = acc + partial[q];
  const float norm = sqrtf(clip_block_sum(acc, lds));
  // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (norm + 1e-6), clamped to at most 1 (a NaN stays a NaN, as torch.clamp's)
  const float c = max_norm / (norm + 1e-6f);
  const bool skip = found_inf && *found_inf != 0.f;   // the step is skipped: Inf x 0 must not put NaNs into the gradients
  const float coef = skip ? 1.f : (c < 1.f ? c : (c == c ? 1.f : c));
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out[0] = norm;
    out[1] = coef;
  }
  if (coef == 1.f) return;                            // nothing to scale: the buffer is not written
  for (size_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    const size_t base = chunk * CLIP_CHUNK;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const size_t i = base + 4 * ((size_t)j * 256 + threadIdx.x);
      if (VEC && i + 4 <= n) {
        f32x4 v = *reinterpret_cast<const f32x4*>(g + i);
        v *= coef;
        *reinterpret_cast<f32x4*>(g + i) = v;
      } else {
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4)
          if (i + c4 < n) g[i + c4] = g[i + c4] * coef;
      }
    }
  }
}

// ---- exponential moving average of the trainable tensors (cara_hip.h: cara_ema_update) ----
// adamw_kernel's scheme once more: pointers and sizes of up to 32 tensors BY VALUE in the kernel arguments (784 bytes), a prefix walk,
// 1024-element chunks -- one launch over the 14 tensors of a step, no table in device memory.
struct ema_table {
  float* e[CARA_ADAMW_MAX_TENSORS];
  const float* p[CARA_ADAMW_MAX_TENSORS];
  size_t n[CARA_ADAMW_MAX_TENSORS];
  int ntensors;
  float weight;              // 1 - decay, used when weight_dev is NULL
  const float* weight_dev;   // the capturable form: the weight lives in device memory
};

// torch.lerp's two-branch definition, every operation a single IEEE fp32 operation (no fma: see the clip kernels above)
__device__ __forceinline__ float ema_lerp(float e, float p, float w, float one_minus_w) {
#pragma clang fp contract(off)
  const float d = p - e;
  if (w < 0.5f) {
    const float s = w * d;
    return e + s;
  }
  const float s = d * one_minus_w;
  return p - s;
}

__global__ __launch_bounds__(256) void ema_kernel(const ema_table a) {
#pragma clang fp contract(off)
  int t = 0, first = 0;
  for (; t < a.ntensors && t < CARA_ADAMW_MAX_TENSORS; ++t) {
    const int nchunk = (int)((a.n[t] + ADAMW_CHUNK - 1) / ADAMW_CHUNK);
    if ((int)blockIdx.x < first + nchunk) break;
    first += nchunk;
  }
  if (t >= a.ntensors || t >= CARA_ADAMW_MAX_TENSORS) return;
  const float w = a.weight_dev ? *a.weight_dev : a.weight;
  if (!(w >= 0.f && w <= 1.f)) return;   // a device weight outside [0, 1], or a NaN: nothing is written
  const float omw = 1.f - w;             // exact for w in [0.5, 1], the only range that reads it
  float* e = a.e[t];
  const float* p = a.p[t];
  const size_t n = a.n[t];
  const size_t base = (size_t)((int)blockIdx.x - first) * ADAMW_CHUNK;
  if ((((uintptr_t)e | (uintptr_t)p) & 15) == 0) {   // both 16-byte aligned: one float4 per thread (the chunk base is a multiple of 4)
    const size_t i = base + 4 * (size_t)threadIdx.x;
    if (i + 4 <= n) {
      f32x4 ev = *reinterpret_cast<const f32x4*>(e + i);
      const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
#pragma unroll
      for (int c = 0; c < 4; ++c) ev[c] = ema_lerp(ev[c], pv[c], w, omw);
      *reinterpret_cast<f32x4*>(e + i) = ev;
    } else {
      for (size_t k = i; k < n; ++k) e[k] = ema_lerp(e[k], p[k], w, omw);   // the tensor's last 1 .. 3 elements
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const size_t i = base + (size_t)j * 256 + threadIdx.x;
    if (i < n) e[i] = ema_lerp(e[i], p[i], w, omw);
  }
}

// ---- sharpness-aware minimisation: the move to w + rho g / |g| and the way back (cara_hip.h: cara_sam_perturb, cara_sam_restore) ----
// ema_kernel's scheme a third time: pointers and sizes of up to 32 tensors BY VALUE in the kernel arguments (1064 bytes), a prefix walk,
// 1024-element chunks -- one launch over the 14 tensors of a step.  Both launches move 0.5 MB at rank 16: their cost is the launch.
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

struct sam_table {
  float* p[CARA_ADAMW_MAX_TENSORS];
  const float* g[CARA_ADAMW_MAX_TENSORS];   // (restore: unused)
  float* b[CARA_ADAMW_MAX_TENSORS];         // perturb writes the backup, restore reads it
  size_t n[CARA_ADAMW_MAX_TENSORS];
  int ntensors;
  float rho;
  const float* norm;
  const float* found_inf_in;                // perturb: the carry it reads (or NULL)
  float* found_inf_out;                     // restore: the word the carry is added to (or NULL)
  float* state;
};

// one fp32 multiply, then one fp32 add: tests/sam_model.py restates exactly this (no fma: see the clip kernels above)
__device__ __forceinline__ float sam_move(float p, float g, float scale) {
#pragma clang fp contract(off)
  const float s = scale * g;
  return p + s;
}

// -> the tensor of this workgroup and the first element of its chunk, or -1 past the last tensor (uniform)
__device__ __forceinline__ int sam_locate(const sam_table& a, size_t* base) {
  int t = 0, first = 0;
  for (; t < a.ntensors && t < CARA_ADAMW_MAX_TENSORS; ++t) {
    const int nchunk = (int)((a.n[t] + ADAMW_CHUNK - 1) / ADAMW_CHUNK);
    if ((int)blockIdx.x < first + nchunk) break;
    first += nchunk;
  }
  if (t >= a.ntensors || t >= CARA_ADAMW_MAX_TENSORS) return -1;
  *base = (size_t)((int)blockIdx.x - first) * ADAMW_CHUNK;
  return t;
}

__global__ __launch_bounds__(256) void sam_perturb_kernel(const sam_table a) {
#pragma clang fp contract(off)
  size_t base = 0;
  const int t = sam_locate(a, &base);
  if (t < 0) return;
  // every thread forms the same scale from the same two device floats: two IEEE operations
  const float carry = a.found_inf_in ? *a.found_inf_in : 0.f;
  const float norm = *a.norm;
  const bool move = !(carry != 0.f) && __builtin_isfinite(norm);   // an overflowed first pass, or a norm that is none: only the backup
  const float den = norm + 1e-12f;
  const float scale = move ? a.rho / den : 0.f;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.state[0] = carry;
    a.state[1] = norm;
    a.state[2] = scale;
    a.state[3] = 0.f;
  }
  float* p = a.p[t];
  const float* g = a.g[t];
  float* b = a.b[t];
  const size_t n = a.n[t];
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)b) & 15) == 0) {   // all three 16-byte aligned: one float4 per thread
    const size_t i = base + 4 * (size_t)threadIdx.x;
    if (i + 4 <= n) {
      f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
      *reinterpret_cast<f32x4*>(b + i) = pv;
      if (move) {
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
        for (int c = 0; c < 4; ++c) pv[c] = sam_move(pv[c], gv[c], scale);
        *reinterpret_cast<f32x4*>(p + i) = pv;
      }
    } else {
      for (size_t k = i; k < n; ++k) {   // the tensor's last 1 .. 3 elements
        const float pk = p[k];
        b[k] = pk;
        if (move) p[k] = sam_move(pk, g[k], scale);
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const size_t i = base + (size_t)j * 256 + threadIdx.x;
    if (i < n) {
      const float pi = p[i];
      b[i] = pi;
      if (move) p[i] = sam_move(pi, g[i], scale);
    }
  }
}

// p = backup: a copy of the bits (dwords moved, never an arithmetic operation: -0, subnormals and NaN payloads come back)
__global__ __launch_bounds__(256) void sam_restore_kernel(const sam_table a) {
  size_t base = 0;
  const int t = sam_locate(a, &base);
  if (t < 0) return;
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.found_inf_out) *a.found_inf_out += a.state[0];   // the first pass's overflow, once
  unsigned* p = reinterpret_cast<unsigned*>(a.p[t]);
  const unsigned* b = reinterpret_cast<const unsigned*>(a.b[t]);
  const size_t n = a.n[t];
  if ((((uintptr_t)p | (uintptr_t)b) & 15) == 0) {
    const size_t i = base + 4 * (size_t)threadIdx.x;
    if (i + 4 <= n) {
      *reinterpret_cast<u32x4*>(p + i) = *reinterpret_cast<const u32x4*>(b + i);
    } else {
      for (size_t k = i; k < n; ++k) p[k] = b[k];
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const size_t i = base + (size_t)j * 256 + threadIdx.x;
    if (i < n) p[i] = b[i];
  }
}

// the checks the two entries share -> the launch's workgroups, 0 for CARA_E_ARG
size_t sam_fill(sam_table& a, int ntensors, float* const* param, const float* const* grad, float* const* backup, const size_t* n) {
  if (!param || !backup || !n || ntensors < 1 || ntensors > CARA_ADAMW_MAX_TENSORS) return 0;
  size_t chunks = 0;
  for (int t = 0; t < ntensors; ++t) {
    const float* g = grad ? grad[t] : nullptr;
    if (!param[t] || !backup[t] || (grad && !g) || n[t] == 0 || ((uintptr_t)param[t] | (uintptr_t)backup[t] | (uintptr_t)g) % 4 != 0) return 0;
    if (n[t] > (size_t)0x7fffffffu * ADAMW_CHUNK) return 0;
    // backup[t] overlapping param[t] or grad[t] anywhere in its n[t] elements (pointer equality is the common mistake)
    const uintptr_t lo = (uintptr_t)backup[t], bytes = n[t] * sizeof(float), pp = (uintptr_t)param[t], gg = (uintptr_t)g;
    if ((lo < pp + bytes && pp < lo + bytes) || (gg && lo < gg + bytes && gg < lo + bytes)) return 0;
    a.p[t] = param[t];
    a.g[t] = g;
    a.b[t] = backup[t];
    a.n[t] = n[t];
    chunks += (n[t] + ADAMW_CHUNK - 1) / ADAMW_CHUNK;
  }
  if (chunks > 0x7fffffffu) return 0;
  a.ntensors = ntensors;
  return chunks;
}

}  // namespace

extern "C" int cara_sam_perturb(int ntensors, float* const* param, const float* const* grad, float* const* backup, const size_t* n,
                                float rho, const float* norm, const float* found_inf, float* state, void* stream) {
  if (!grad || !norm || !state || !(rho >= 0.f) || !__builtin_isfinite(rho)) return CARA_E_ARG;   // (a NaN fails the comparison)
  if (((uintptr_t)norm | (uintptr_t)found_inf | (uintptr_t)state) % 4 != 0) return CARA_E_ARG;
  sam_table a = {};
  const size_t chunks = sam_fill(a, ntensors, param, grad, backup, n);
  if (chunks == 0) return CARA_E_ARG;
  a.rho = rho;
  a.norm = norm;
  a.found_inf_in = found_inf;
  a.state = state;
  hipLaunchKernelGGL(sam_perturb_kernel, dim3((unsigned)chunks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}

extern "C" int cara_sam_restore(int ntensors, float* const* param, const float* const* backup, const size_t* n, const float* state,
                                float* found_inf, void* stream) {
  if (!state || ((uintptr_t)state | (uintptr_t)found_inf) % 4 != 0) return CARA_E_ARG;
  sam_table a = {};
  const size_t chunks = sam_fill(a, ntensors, param, nullptr, const_cast<float* const*>(backup), n);
  if (chunks == 0) return CARA_E_ARG;
  a.found_inf_out = found_inf;
  a.state = const_cast<float*>(state);
  hipLaunchKernelGGL(sam_restore_kernel, dim3((unsigned)chunks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}

extern "C" int cara_ema_update(int ntensors, float* const* ema, const float* const* param, const size_t* n, float weight,
                               const float* weight_dev, void* stream) {
  if (!ema || !param || !n || ntensors < 1 || ntensors > CARA_ADAMW_MAX_TENSORS) return CARA_E_ARG;
  if (weight_dev ? (uintptr_t)weight_dev % 4 != 0 : !(weight >= 0.f && weight <= 1.f)) return CARA_E_ARG;   // (a NaN fails the comparison)
  ema_table a = {};
  size_t chunks = 0;
  for (int t = 0; t < ntensors; ++t) {
    if (!ema[t] || !param[t] || n[t] == 0 || ((uintptr_t)ema[t] | (uintptr_t)param[t]) % 4 != 0 || ema[t] == param[t]) return CARA_E_ARG;
    if (n[t] > (size_t)0x7fffffffu * ADAMW_CHUNK) return CARA_E_ARG;
    a.e[t] = ema[t];
    a.p[t] = param[t];
    a.n[t] = n[t];
    chunks += (n[t] + ADAMW_CHUNK - 1) / ADAMW_CHUNK;
  }
  if (chunks > 0x7fffffffu) return CARA_E_ARG;
  a.ntensors = ntensors;
  a.weight = weight;
  a.weight_dev = weight_dev;
  hipLaunchKernelGGL(ema_kernel, dim3((unsigned)chunks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}

extern "C" int cara_amp_update(float* state, const float* found_inf, float growth, float backoff, int interval, float max_scale,
                               void* stream) {
  if (!state || !found_inf || !(growth >= 1.f) || !(backoff > 0.f && backoff <= 1.f) || interval <= 0 || !(max_scale >= 1.f)) return CARA_E_ARG;
  hipLaunchKernelGGL(amp_update_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), state, found_inf, growth, backoff,
                     interval, max_scale);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}

extern "C" int cara_adamw_step(const cara_adamw_args* a, void* stream) {
  if (!a || a->ntensors <= 0 || a->ntensors > CARA_ADAMW_MAX_TENSORS || (a->step <= 0 && !a->dyn)) return CARA_E_ARG;
  size_t chunks = 0;
  for (int t = 0; t < a->ntensors; ++t) {
    const cara_adamw_tensor& T = a->t[t];
    if (!T.p || !T.g || !T.m || !T.v || T.n == 0 || T.group < 0 || T.group >= CARA_ADAMW_MAX_GROUPS) return CARA_E_ARG;
    chunks += (T.n + ADAMW_CHUNK - 1) / ADAMW_CHUNK;
  }
  if (chunks > 0x7fffffffu) return CARA_E_ARG;
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)chunks), dim3(256), 0, static_cast<hipStream_t>(stream), *a);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}

extern "C" int cara_grad_accumulate(float* dst, const float* a, const float* b, size_t n, void* stream) {
  if (!dst || !a || n == 0 || ((uintptr_t)dst | (uintptr_t)a | (uintptr_t)b) % 4 != 0) return CARA_E_ARG;
  const uintptr_t r = (uintptr_t)dst % 16;
  size_t head = 0, nvec = 0;
  if ((uintptr_t)a % 16 == r && (!b || (uintptr_t)b % 16 == r)) {
    head = ((16 - r) % 16) / 4;
    if (head > n) head = n;
    nvec = (n - head) / 4;
  }
  const size_t edge = n - 4 * nvec, work = nvec > edge ? nvec : edge;
  size_t grid = (work + 255) / 256;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(grad_accumulate_kernel, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), dst, a, b, n, head,
                     nvec);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}

extern "C" size_t cara_grad_clip_scratch_bytes(size_t n) {
  if (n == 0 || n > ((size_t)1 << 31)) return 0;
  return ((n + CLIP_CHUNK - 1) / CLIP_CHUNK) * sizeof(float);
}

extern "C" int cara_grad_clip(float* g, size_t n, float max_norm, float* scratch, const float* found_inf, float* out, void* stream) {
  if (!g || !scratch || !out || n == 0 || n > ((size_t)1 << 31) || !(max_norm > 0.f) || (uintptr_t)g % 4 != 0) return CARA_E_ARG;
  const size_t chunks = (n + CLIP_CHUNK - 1) / CLIP_CHUNK;                 // <= 2^18
  const unsigned grid2 = (unsigned)(chunks < (size_t)CLIP_MAX_GRID ? chunks : (size_t)CLIP_MAX_GRID);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if ((uintptr_t)g % 16 == 0) {
    hipLaunchKernelGGL(grad_sumsq_kernel<true>, dim3((unsigned)chunks), dim3(256), 0, st, g, n, scratch);
    hipLaunchKernelGGL(grad_scale_kernel<true>, dim3(grid2), dim3(256), 0, st, g, n, chunks, max_norm, scratch, found_inf, out);
  } else {   // a buffer that is only 4-byte aligned: the same element-to-thread map and summation order with dword accesses
    hipLaunchKernelGGL(grad_sumsq_kernel<false>, dim3((unsigned)chunks), dim3(256), 0, st, g, n, scratch);
    hipLaunchKernelGGL(grad_scale_kernel<false>, dim3(grid2), dim3(256), 0, st, g, n, chunks, max_norm, scratch, found_inf, out);
  }
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}
