// Scoring a batch of logits on the device (gfx950): what `test()` of image_classification/vit_cp.py:73-82 does with
// `out.argmax(1) == y` and one `.item()` per batch, as ONE launch per batch that adds into a 40-byte device-resident
// state -- no host read until the caller wants the totals.
//
// state = five 64-bit words (cara_eval_state_bytes):
//   [0] int64  rows scored            [1] int64  top-1 hits           [2] int64  top-5 hits
//   [3] double sum of the per-row cross-entropy                       [4] int64  rows whose label is outside [0, classes)
// A row with a bad label raises word 4 and adds to nothing else.
//
// Per row, with v = logits[label]:  rank = #{c : l[c] > v} + #{c < label : l[c] == v}  is the position of the label in a
// stable descending sort, so  top-1 <=> rank == 0  (ties go to the lowest class index, numpy.argmax's rule) and
// top-5 <=> rank < 5  (always, with fewer than five classes).  Cross-entropy = m + log(sum exp(l - m)) - v with the
// log-sum-exp in fp32 (as cara_cross_entropy forms it; the accurate expf / logf here, not the fast intrinsics: the kernel
// is bound by its loads); rows are summed in fp64.
//
// One wave per row: pass 1 the row maximum, pass 2 (the row is in L2 by then: at most 87 KB) the exponentials and the
// rank, 16-byte loads where the row is 16-byte aligned.  A workgroup of four waves walks rows with a grid stride, adds
// its waves' partial sums in LDS and issues one atomicAdd per non-zero word.
//
// cara_eval_accumulate_report is the same kernel body with REPORT = true: the confusion matrix and the calibration bins of
// include/cara_hip.h.  pass 2 also carries the lowest index whose logit equals the maximum (a wave-min reduction), the
// confidence is the reciprocal of the sum the loss already forms.  The plain entry launches the REPORT = false instantiation.
#include "common.h"

namespace {

constexpr int EVAL_WAVES = 4;

// REPORT adds the lowest class index that holds the row maximum (the predicted class) to what a lane carries
template <bool REPORT>
struct RowAcc {
  float s;
  int rank;
};
template <>
struct RowAcc<true> {
  float s;
  int rank;
  int pred;
};

template <bool REPORT>
__device__ __forceinline__ void row_term(float x, int c, float m, float v, int y, RowAcc<REPORT>& a) {
  a.s += expf(x - m);
  a.rank += (x > v || (x == v && c < y)) ? 1 : 0;
  if constexpr (REPORT) a.pred = (x == m && c < a.pred) ? c : a.pred;
}

// The walk over one row that every scoring kernel of this file shares (the accumulate kernel, its report form and the predict
// kernel): the SAME loads in the SAME order, so the three form the same maximum and, bit for bit, the same sum.  16-byte loads over
// the first 4 * C4 classes when the row starts on 16 bytes (C4 = 0 otherwise), a scalar tail, lane-strided.
__device__ __forceinline__ int row_vec4(const float* lr, int C) { return (reinterpret_cast<uintptr_t>(lr) & 15) == 0 ? C >> 2 : 0; }

// pass 1: the row maximum, in every lane (never below -3e38: a row without a finite maximum keeps that value)
__device__ __forceinline__ float row_max(const float* __restrict__ lr, int C, int C4, int lane) {
  float m = -3.0e38f;
  for (int i = lane; i < C4; i += 64) {
    const float4 q = reinterpret_cast<const float4*>(lr)[i];
    m = fmaxf(fmaxf(m, q.x), fmaxf(q.y, fmaxf(q.z, q.w)));
  }
  for (int c = C4 * 4 + lane; c < C; c += 64) m = fmaxf(m, lr[c]);
  return wave_max(m);
}

// pass 2: this lane's part of sum expf(l - m) and of the rank of (v, y) -- the caller reduces both over the wave
template <bool REPORT>
__device__ __forceinline__ RowAcc<REPORT> row_walk(const float* __restrict__ lr, int C, int C4, int lane, float m, float v, int y) {
  RowAcc<REPORT> a;
  a.s = 0.f;
  a.rank = 0;
  if constexpr (REPORT) a.pred = C;
  for (int i = lane; i < C4; i += 64) {
    const float4 q = reinterpret_cast<const float4*>(lr)[i];
    row_term(q.x, 4 * i, m, v, y, a);
    row_term(q.y, 4 * i + 1, m, v, y, a);
    row_term(q.z, 4 * i + 2, m, v, y, a);
    row_term(q.w, 4 * i + 3, m, v, y, a);
  }
  for (int c = C4 * 4 + lane; c < C; c += 64) row_term(lr[c], c, m, v, y, a);
  return a;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// REPORT = false: cara_eval_accumulate, `report` and `bins` unused.  REPORT = true: cara_eval_accumulate_report -- per row one
// atomicAdd on the confusion cell (scattered: nothing to stage) and the three bin words of its confidence bin added up per
// workgroup in LDS, published with one atomic per non-empty bin word.
template <bool REPORT>
__global__ __launch_bounds__(EVAL_WAVES * 64) void eval_accumulate_kernel(const float* __restrict__ logits, int ldl,
                                                                          const int64_t* __restrict__ labels, int n_valid,
                                                                          int C, unsigned long long* __restrict__ state,
                                                                          unsigned long long* __restrict__ report, int bins) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ unsigned int sh_cnt[REPORT ? CARA_EVAL_REPORT_MAX_BINS : 1], sh_hit[REPORT ? CARA_EVAL_REPORT_MAX_BINS : 1];
  __shared__ double sh_conf[REPORT ? CARA_EVAL_REPORT_MAX_BINS : 1];
  if constexpr (REPORT) {
    if ((int)threadIdx.x < bins) {
      sh_cnt[threadIdx.x] = 0; sh_hit[threadIdx.x] = 0;
      sh_conf[threadIdx.x] = 0.0;
    }
    __syncthreads();
  }
  unsigned long long n = 0, t1 = 0, t5 = 0, bad = 0;
  double loss = 0.0;
  for (int b = blockIdx.x * EVAL_WAVES + wave; b < n_valid; b += gridDim.x * EVAL_WAVES) {
    const int64_t y64 = labels[b];
    if (y64 < 0 || y64 >= C) {   // (wave-uniform: one row per wave)
      ++bad;
      continue;
    }
    const int y = (int)y64;
    const float* lr = logits + (size_t)b * ldl;
    const int C4 = row_vec4(lr, C);
    const float m = row_max(lr, C, C4, lane);
    const float v = lr[y];
    const RowAcc<REPORT> a = row_walk<REPORT>(lr, C, C4, lane, m, v, y);
    const float s = wave_sum(a.s);
    const int rank = wave_sum_int(a.rank);
    const float lse = m + logf(s);
    ++n;
    t1 += rank == 0 ? 1 : 0;
    t5 += rank < 5 ? 1 : 0;
    loss += (double)lse - (double)v;
    if constexpr (REPORT) {
      int pred = a.pred;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) pred = min(pred, __shfl_xor(pred, o, 64));
      // a row without a finite maximum (NaN, or nothing above -3e38) matches no class: it is counted in column 0 / bin 0,
      // never outside the buffer
      pred = pred < C ? pred : 0;
      const float conf = 1.0f / s, fb = conf * (float)bins;
      const int bin = fb >= (float)(bins - 1) ? bins - 1 : (fb > 0.f ? (int)fb : 0);
      if (lane == 0) {
        atomicAdd(report + (size_t)y * C + pred, 1ull);
        atomicAdd(&sh_cnt[bin], 1u);
        if (rank == 0) atomicAdd(&sh_hit[bin], 1u);
        atomicAdd(&sh_conf[bin], (double)conf);
      }
    }
  }
  // every lane of a wave holds the wave's totals: lane 0 of each wave publishes them, thread 0 adds the four
  __shared__ unsigned long long sh_i[EVAL_WAVES][4];
  __shared__ double sh_l[EVAL_WAVES];
  if (lane == 0) {
    sh_i[wave][0] = n; sh_i[wave][1] = t1; sh_i[wave][2] = t5; sh_i[wave][3] = bad;
    sh_l[wave] = loss;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < EVAL_WAVES; ++w) {
      n += sh_i[w][0]; t1 += sh_i[w][1]; t5 += sh_i[w][2]; bad += sh_i[w][3];
      loss += sh_l[w];
    }
    if (n) {
      atomicAdd(state + 0, n);
      atomicAdd(reinterpret_cast<double*>(state + 3), loss);
    }
    if (t1) atomicAdd(state + 1, t1);
    if (t5) atomicAdd(state + 2, t5);
    if (bad) atomicAdd(state + 4, bad);
  }
  if constexpr (REPORT) {
    // (the LDS adds above are ordered before this by the __syncthreads every wave has passed)
    const int t = threadIdx.x;
    if (t < bins && sh_cnt[t]) {
      unsigned long long* bin_words = report + (size_t)C * C;
      atomicAdd(bin_words + t, (unsigned long long)sh_cnt[t]);
      if (sh_hit[t]) atomicAdd(bin_words + bins + t, (unsigned long long)sh_hit[t]);
      atomicAdd(reinterpret_cast<double*>(bin_words + 2 * bins) + t, sh_conf[t]);
    }
  }
}

// what every scoring entry asks of the logit table (cara_eval_predict takes its labels as optional and has no state)
bool eval_table_ok(const float* logits, int ldl, int B, int n_valid, int classes) {
  if (!logits || B <= 0 || n_valid < 0 || n_valid > B || classes < 1 || ldl < classes) return false;
  return (reinterpret_cast<uintptr_t>(logits) & 3) == 0;
}

bool eval_args_ok(const float* logits, int ldl, const int64_t* labels, int B, int n_valid, int classes, void* state) {
  if (!eval_table_ok(logits, ldl, B, n_valid, classes) || !labels || !state) return false;
  return (reinterpret_cast<uintptr_t>(state) & 7) == 0;
}

// at most 256 workgroups (one per CU): 1 280 atomics per launch at the worst, every row still read once
int eval_grid(int n_valid) {
  const int grid = (n_valid + EVAL_WAVES - 1) / EVAL_WAVES;
  return grid > 256 ? 256 : grid;
}

// ---- cara_eval_combine_views: the V views' logits of a sample -> one row that the two kernels above score unchanged ----------
// One wave per sample.  Pass 1 walks the V rows (V <= 16) as the accumulate kernel walks one: row maximum, then lse_v = m_v +
// logf(sum expf(l - m_v)); lane v keeps lse_v and pass 2 reads it with v_readlane (v is wave-uniform; the read does not depend on
// which lanes are active) -- no LDS, no barrier: the waves of a workgroup run different trip counts.  Pass 2 is over the classes:
// per class the V values are read twice (L1 / L2: a sample is at most 64 KB at 1000 classes), once for M = max_v a_v and once for
// the sum of expf(a_v - M) in view order.  16-byte loads when every row of the sample is 16-byte aligned, the output row stored
// 16 bytes at a time when it is too.
__device__ __forceinline__ float lane_value(float x, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); }

template <int MODE>
__device__ __forceinline__ float combine_one(const float* __restrict__ col, int ldl, int V, float my_lse, float logV, float fV) {
  if constexpr (MODE == CARA_EVAL_COMBINE_LOGIT) {
    float acc = col[0];
    for (int v = 1; v < V; ++v) acc += col[(size_t)v * ldl];
    return acc / fV;
  } else {
    float M = -INFINITY;
    for (int v = 0; v < V; ++v) M = fmaxf(M, col[(size_t)v * ldl] - lane_value(my_lse, v));
    float t = 0.f;
    for (int v = 0; v < V; ++v) t += expf((col[(size_t)v * ldl] - lane_value(my_lse, v)) - M);
    // M = -inf: the class has probability zero in every view (t is NaN there: -inf - -inf)
    return M == -INFINITY ? M : (M + logf(t)) - logV;
  }
}

template <int MODE>
__global__ __launch_bounds__(EVAL_WAVES * 64) void eval_combine_kernel(const float* __restrict__ logits, int ldl, int S, int V, int C,
                                                                       float* __restrict__ out, int ldo) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float fV = (float)V, logV = logf(fV);
  for (int s = blockIdx.x * EVAL_WAVES + wave; s < S; s += gridDim.x * EVAL_WAVES) {
    const float* base = logits + (size_t)s * V * ldl;
    float* orow = out + (size_t)s * ldo;
    // every row of the sample starts on 16 bytes: the first does and the stride keeps it (one view: no stride to keep)
    const bool vec = ((reinterpret_cast<uintptr_t>(base) & 15) == 0) && (V == 1 || (ldl & 3) == 0);
    const bool vec_out = (reinterpret_cast<uintptr_t>(orow) & 15) == 0;
    const int C4 = vec ? C >> 2 : 0;
    float my_lse = 0.f;
    if constexpr (MODE == CARA_EVAL_COMBINE_PROB) {
      for (int v = 0; v < V; ++v) {
        const float* lr = base + (size_t)v * ldl;
        float m = -INFINITY;
        for (int i = lane; i < C4; i += 64) {
          const float4 q = reinterpret_cast<const float4*>(lr)[i];
          m = fmaxf(fmaxf(m, q.x), fmaxf(q.y, fmaxf(q.z, q.w)));
        }
        for (int c = C4 * 4 + lane; c < C; c += 64) m = fmaxf(m, lr[c]);
        m = wave_max(m);
        float sum = 0.f;
        for (int i = lane; i < C4; i += 64) {
          const float4 q = reinterpret_cast<const float4*>(lr)[i];
          sum += expf(q.x - m);
          sum += expf(q.y - m);
          sum += expf(q.z - m);
          sum += expf(q.w - m);
        }
        for (int c = C4 * 4 + lane; c < C; c += 64) sum += expf(lr[c] - m);
        const float lse = m + logf(wave_sum(sum));   // (the same value in every lane)
        my_lse = lane == v ? lse : my_lse;
      }
    }
    for (int i = lane; i < C4; i += 64) {
      float4 o;
      o.x = combine_one<MODE>(base + 4 * i, ldl, V, my_lse, logV, fV);
      o.y = combine_one<MODE>(base + 4 * i + 1, ldl, V, my_lse, logV, fV);
      o.z = combine_one<MODE>(base + 4 * i + 2, ldl, V, my_lse, logV, fV);
      o.w = combine_one<MODE>(base + 4 * i + 3, ldl, V, my_lse, logV, fV);
      if (vec_out) {
        reinterpret_cast<float4*>(orow)[i] = o;
      } else {
        orow[4 * i] = o.x; orow[4 * i + 1] = o.y; orow[4 * i + 2] = o.z; orow[4 * i + 3] = o.w;
      }
    }
    for (int c = C4 * 4 + lane; c < C; c += 64) orow[c] = combine_one<MODE>(base + c, ldl, V, my_lse, logV, fV);
  }
}

// ---- cara_eval_predict: a batch of logit rows -> per-sample records in a device table (include/cara_hip.h) ---------------------
// One wave per row, rows walked with the accumulate kernel's grid stride.  Passes 1 and 2 are row_max / row_walk above, so m, s and
// the rank are the accumulate kernel's own.  Then k selection rounds over the row (L1 / L2 by now: at most 16 KB at 4096 classes):
// a lane keeps the best (value, index) pair of its classes among those that sort AFTER the previous pick in the stable descending
// order -- value below it, or equal with a higher index --, a six-stage xor butterfly over the pairs leaves the wave's best in every
// lane, and lane j keeps round j's.  Comparisons only: a NaN is never picked, -inf is picked like any value.  No LDS, no barrier
// (the waves of a workgroup run different trip counts), no atomics: lanes 0..k-1 store the k indices and the k probabilities of the
// row as two coalesced stores, lane 0 its loss and rank.
struct Pick {
  float x;
  int c;
};

// (x, c) sorts before (bx, bc) in the stable descending order
__device__ __forceinline__ bool sorts_before(float x, int c, float bx, int bc) { return x > bx || (x == bx && c < bc); }

__device__ __forceinline__ void pick_term(float x, int c, const Pick& prev, Pick& best) {
  const bool open = sorts_before(prev.x, prev.c, x, c);           // behind the previous pick
  if (open && sorts_before(x, c, best.x, best.c)) {
    best.x = x;
    best.c = c;
  }
}

// `none` = classes: no class is left (or the rest are NaN).  -inf with index `none` loses against every real candidate.
__device__ __forceinline__ Pick next_pick(const float* __restrict__ lr, int C, int C4, int lane, const Pick& prev) {
  Pick best = {-INFINITY, C};
  for (int i = lane; i < C4; i += 64) {
    const float4 q = reinterpret_cast<const float4*>(lr)[i];
    pick_term(q.x, 4 * i, prev, best);
    pick_term(q.y, 4 * i + 1, prev, best);
    pick_term(q.z, 4 * i + 2, prev, best);
    pick_term(q.w, 4 * i + 3, prev, best);
  }
  for (int c = C4 * 4 + lane; c < C; c += 64) pick_term(lr[c], c, prev, best);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ox = __shfl_xor(best.x, o, 64);
    const int oc = __shfl_xor(best.c, o, 64);
    if (sorts_before(ox, oc, best.x, best.c)) {
      best.x = ox;
      best.c = oc;
    }
  }
  return best;
}

__global__ __launch_bounds__(EVAL_WAVES * 64) void eval_predict_kernel(const float* __restrict__ logits, int ldl,
                                                                       const int64_t* __restrict__ labels, int n_valid, int C, int k,
                                                                       int64_t first, int32_t* __restrict__ topk_idx,
                                                                       float* __restrict__ topk_prob, float* __restrict__ loss_out,
                                                                       int32_t* __restrict__ rank_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = blockIdx.x * EVAL_WAVES + wave; b < n_valid; b += gridDim.x * EVAL_WAVES) {
    const float* lr = logits + (size_t)b * ldl;
    const int C4 = row_vec4(lr, C);
    const float m = row_max(lr, C, C4, lane);
    // no labels, or a label outside [0, classes): v = NaN compares false with everything, the walk still forms the same sum
    bool labelled = false;
    int y = 0;
    if (labels) {
      const int64_t y64 = labels[b];   // (wave-uniform: one row per wave)
      labelled = y64 >= 0 && y64 < C;
      y = labelled ? (int)y64 : 0;
    }
    const float v = labelled ? lr[y] : __int_as_float(0x7fc00000);
    const RowAcc<false> a = row_walk<false>(lr, C, C4, lane, m, v, y);
    const float s = wave_sum(a.s);
    const int rank = wave_sum_int(a.rank);
    Pick prev = {INFINITY, -1}, mine = {-INFINITY, C};
    bool finite_max = false;
    for (int j = 0; j < k; ++j) {
      const Pick p = next_pick(lr, C, C4, lane, prev);
      if (j == 0) finite_max = p.c < C && p.x == m;   // the report kernel's rule: some class holds the maximum
      if (lane == j) mine = p;
      if (p.c >= C) break;                            // nothing is left: the later slots keep index -1
      prev = p;
    }
    const size_t row = (size_t)(first + b);
    if (lane < k) {
      int idx = mine.c < C ? mine.c : -1;
      float prob = mine.c < C ? expf(mine.x - m) / s : 0.f;
      if (!finite_max) {
        idx = lane == 0 ? 0 : -1;
        prob = __int_as_float(0x7fc00000);
      }
      topk_idx[row * k + lane] = idx;
      topk_prob[row * k + lane] = prob;
    }
    if (labels && lane == 0) {
      const float nan = __int_as_float(0x7fc00000);
      loss_out[row] = labelled && finite_max ? (float)((double)(m + logf(s)) - (double)v) : nan;
      rank_out[row] = labelled ? rank : -1;
    }
  }
}

}  // namespace

extern "C" int cara_eval_predict(const float* logits, int ldl, const int64_t* labels, int B, int n_valid, int classes, int k,
                                 int64_t first, int64_t n_rows, int32_t* topk_idx, float* topk_prob, float* loss, int32_t* rank,
                                 void* stream) {
  if (!eval_table_ok(logits, ldl, B, n_valid, classes) || !topk_idx || !topk_prob) return CARA_E_ARG;
  if ((labels != nullptr) != (loss != nullptr) || (labels != nullptr) != (rank != nullptr)) return CARA_E_ARG;
  if (k < 1 || k > CARA_EVAL_PREDICT_MAX_K || first < 0 || n_rows < 0 || first > n_rows - n_valid) return CARA_E_ARG;
  const uintptr_t four = reinterpret_cast<uintptr_t>(topk_idx) | reinterpret_cast<uintptr_t>(topk_prob) |
                         reinterpret_cast<uintptr_t>(loss) | reinterpret_cast<uintptr_t>(rank);
  if ((four & 3) || (reinterpret_cast<uintptr_t>(labels) & 7)) return CARA_E_ARG;
  if (n_valid == 0) return CARA_OK;
  hipLaunchKernelGGL(eval_predict_kernel, dim3(eval_grid(n_valid)), dim3(EVAL_WAVES * 64), 0, static_cast<hipStream_t>(stream), logits,
                     ldl, labels, n_valid, classes, k, first, topk_idx, topk_prob, loss, rank);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}

extern "C" int cara_eval_combine_views(const float* logits, int ldl, int S, int V, int classes, int mode, float* out, int ldo,
                                       void* stream) {
  if (!logits || !out || S < 1 || V < 1 || V > CARA_EVAL_MAX_VIEWS || classes < 1 || ldl < classes || ldo < classes) return CARA_E_ARG;
  if (mode != CARA_EVAL_COMBINE_PROB && mode != CARA_EVAL_COMBINE_LOGIT) return CARA_E_ARG;
  const uintptr_t lo_l = reinterpret_cast<uintptr_t>(logits), lo_o = reinterpret_cast<uintptr_t>(out);
  if ((lo_l & 3) || (lo_o & 3)) return CARA_E_ARG;
  // the bytes the launch reads and the bytes it writes (the last row of each ends behind its `classes` columns)
  const uintptr_t hi_l = lo_l + (((size_t)S * V - 1) * (size_t)ldl + classes) * sizeof(float);
  const uintptr_t hi_o = lo_o + (((size_t)S - 1) * (size_t)ldo + classes) * sizeof(float);
  if (lo_o < hi_l && lo_l < hi_o) return CARA_E_ARG;
  const dim3 grid(eval_grid(S)), block(EVAL_WAVES * 64);
  if (mode == CARA_EVAL_COMBINE_PROB)
    hipLaunchKernelGGL(eval_combine_kernel<CARA_EVAL_COMBINE_PROB>, grid, block, 0, static_cast<hipStream_t>(stream), logits, ldl, S, V,
                       classes, out, ldo);
  else
    hipLaunchKernelGGL(eval_combine_kernel<CARA_EVAL_COMBINE_LOGIT>, grid, block, 0, static_cast<hipStream_t>(stream), logits, ldl, S, V,
                       classes, out, ldo);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}

extern "C" size_t cara_eval_state_bytes(void) { return 5 * sizeof(unsigned long long); }

extern "C" int cara_eval_accumulate(const float* logits, int ldl, const int64_t* labels, int B, int n_valid, int classes,
                                    void* state, void* stream) {
  if (!eval_args_ok(logits, ldl, labels, B, n_valid, classes, state)) return CARA_E_ARG;
  if (n_valid == 0) return CARA_OK;
  hipLaunchKernelGGL(eval_accumulate_kernel<false>, dim3(eval_grid(n_valid)), dim3(EVAL_WAVES * 64), 0, static_cast<hipStream_t>(stream),
                     logits, ldl, labels, n_valid, classes, static_cast<unsigned long long*>(state),
                     static_cast<unsigned long long*>(nullptr), 0);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}

extern "C" size_t cara_eval_report_bytes(int classes, int bins) {
  if (classes < 1 || classes > CARA_EVAL_REPORT_MAX_CLASSES || bins < 1 || bins > CARA_EVAL_REPORT_MAX_BINS) return 0;
  return ((size_t)classes * classes + 3 * (size_t)bins) * sizeof(unsigned long long);
}

extern "C" int cara_eval_accumulate_report(const float* logits, int ldl, const int64_t* labels, int B, int n_valid, int classes,
                                           void* state, void* report, int bins, void* stream) {
  if (!eval_args_ok(logits, ldl, labels, B, n_valid, classes, state)) return CARA_E_ARG;
  if (cara_eval_report_bytes(classes, bins) == 0 || !report || (reinterpret_cast<uintptr_t>(report) & 7)) return CARA_E_ARG;
  if (n_valid == 0) return CARA_OK;
  hipLaunchKernelGGL(eval_accumulate_kernel<true>, dim3(eval_grid(n_valid)), dim3(EVAL_WAVES * 64), 0, static_cast<hipStream_t>(stream),
                     logits, ldl, labels, n_valid, classes, static_cast<unsigned long long*>(state),
                     static_cast<unsigned long long*>(report), bins);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}
