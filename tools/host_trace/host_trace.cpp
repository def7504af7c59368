// Host trace of libcara_hip.so's whole-model entries: which library calls and which kernel launches cara_vit_forward* and
// cara_vit_backward make, in order, with every argument -- without a GPU.  For refactors of vit.hip's host code: build this program
// against the library before and after (tools/host_trace/trace.sh) and compare the outputs byte for byte.
//
// How: the executable defines the HIP runtime entry points the library imports and the library entries vit.hip calls in other
// translation units.  The executable's definitions take precedence over the shared library's, so every such call lands here, is
// printed, and (library entries) forwarded to the library's own function for its return value and its own launches; the HIP
// stand-ins launch nothing.  All device pointers are made-up addresses that nothing dereferences.  The switches (CARA_*) are read
// once per process by the library: one run per setting.  HOST_TRACE_SITES=1 turns every site bracket on (cara_profile_sites), so the
// event records show the brackets' scopes.  HOST_TRACE_POOL=1 traces the pooled-readout shapes (cara_vit_shape::pool = 1) INSTEAD of the
// token-readout ones, so that the traces of the other settings stay comparable across that feature.
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/cara_hip.h"

// ---- the HIP runtime, as far as the library imports it ----
struct dim3 { unsigned x, y, z; };
typedef void* hipStream_t;
typedef void* hipEvent_t;
typedef int hipError_t;

namespace {
struct Kernel { const void* host; const char* name; };
Kernel* kernels() { static Kernel k[4096]; return k; }
int& nkernels() { static int n = 0; return n; }
const char* kernel_name(const void* host) {
  for (int i = 0; i < nkernels(); ++i)
    if (kernels()[i].host == host) return kernels()[i].name;
  return "?";
}
struct { dim3 grid, block; size_t shmem; hipStream_t stream; } g_cfg;
uintptr_t g_handles = 0xE000;   // events and streams: made-up handles, in order of creation
}  // namespace

extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
  if (nkernels() < 4096) kernels()[nkernels()++] = Kernel{host, device_name};
}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t stream) {
  g_cfg = {grid, block, shmem, stream};
  return 0;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shmem, hipStream_t* stream) {
  *grid = g_cfg.grid; *block = g_cfg.block; *shmem = g_cfg.shmem; *stream = g_cfg.stream;
  return 0;
}
hipError_t hipLaunchKernel(const void* host, dim3 g, dim3 b, void**, size_t shmem, hipStream_t st) {
  printf("    launch %s grid %u,%u,%u block %u,%u,%u lds %zu stream %p\n", kernel_name(host), g.x, g.y, g.z, b.x, b.y, b.z, shmem, st);
  return 0;
}
hipError_t hipGetLastError() { return 0; }
hipError_t hipGetDevice(int* d) { *d = 0; return 0; }
hipError_t hipFuncSetAttribute(const void*, int, int) { return 0; }
hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t st) {
  printf("    memset %p value %d bytes %zu stream %p\n", p, v, n, st);
  return 0;
}
hipError_t hipMemset2DAsync(void* p, size_t pitch, int v, size_t w, size_t h, hipStream_t st) {
  printf("    memset2d %p pitch %zu value %d width %zu height %zu stream %p\n", p, pitch, v, w, h, st);
  return 0;
}
hipError_t hipEventCreate(hipEvent_t* e) { *e = (void*)(g_handles += 0x10); return 0; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = (void*)(g_handles += 0x10); return 0; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = (void*)(g_handles += 0x10); return 0; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return 0; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t st) {
  printf("    event_record %p stream %p\n", e, st);
  return 0;
}
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t e, unsigned flags) {
  printf("    stream_wait stream %p event %p flags %u\n", st, e, flags);
  return 0;
}
}

// ---- printing of arguments ----
namespace {
void put(int v) { printf(" %d", v); }
void put(unsigned v) { printf(" %uu", v); }
void put(long v) { printf(" %ldl", v); }
void put(size_t v) { printf(" %zuz", v); }
void put(float v) { printf(" %a", v); }
void put(bool v) { printf(" %s", v ? "true" : "false"); }
void put(const void* p) { printf(" %p", p); }
void put(const cara_geom* g) {
  if (!g) { printf(" geom:null"); return; }
  printf(" geom{%d %d %d %d %d %a %d}", g->depth, g->dim, g->heads, g->rank, g->Rp, g->scale, g->cp_length);
}
void put(const cara_cp* c) {
  if (!c) { printf(" cp:null"); return; }
  printf(" cp{%p %p %p %p %p %p %p %p %p %p %p %p %p}", (void*)c->A1, (void*)c->A2, (void*)c->A3, (void*)c->A4, (void*)c->P1, (void*)c->P2,
         (void*)c->P3, (void*)c->R1, (void*)c->R2, (void*)c->bias1, (void*)c->bias2, (void*)c->bias3, (void*)c->A5);
}
void put(const cara_layer_grads* l) {
  printf(" lg{%p %p %p %p %p %p %p %p %p %p %p}", (const void*)l->dU_qkv, (const void*)l->dVs_qkv, (const void*)l->dU_proj, (const void*)l->dVs_proj,
         (const void*)l->dU_fc1, (const void*)l->dVs_fc1, (const void*)l->dU_fc2, (const void*)l->dVs_fc2, (const void*)l->dc_proj, (const void*)l->dc_fc1,
         (const void*)l->dc_fc2);
}
void put(const cara_gemm_args* a) {   // byte for byte
  printf(" gemm_args[");
  const unsigned char* b = reinterpret_cast<const unsigned char*>(a);
  for (size_t i = 0; i < sizeof(*a); ++i) printf("%02x", b[i]);
  printf("]");
}
template <class... A>
void enter(const char* name, A... a) {
  printf("  %s(", name);
  (put(a), ...);
  printf(" )\n");
}
template <class R>
R leave(const char* name, R r) {
  printf("  %s -> %lld\n", name, (long long)r);
  return r;
}
}  // namespace

// A library entry: print, forward to the library's own definition (the next one in lookup order), print what it returned.
#define REAL(name) reinterpret_cast<decltype(&name)>(dlsym(RTLD_NEXT, #name))
#define ENTRY(ret, name, params, ...)            \
  ret name params {                              \
    enter(#name, __VA_ARGS__);                   \
    return leave(#name, REAL(name)(__VA_ARGS__)); \
  }

extern "C" {
ENTRY(int, cara_factor_prep, (const cara_geom* g, const cara_cp* cp, const float* b1, const float* b2, const float* b3, void* pack, void* stream),
      g, cp, b1, b2, b3, pack, stream)
ENTRY(int, cara_dense_delta_materialize, (const cara_geom* g, const cara_cp* cp, void* Dm, void* Dmt, void* stream), g, cp, Dm, Dmt, stream)
ENTRY(int, cara_im2col_patches, (const float* img, void* patches, int B, int C, int Hi, int Wi, int p, void* stream), img, patches, B, C, Hi, Wi, p, stream)
ENTRY(int, cara_im2col_patches_u8, (const unsigned char* px, const float* mean, const float* sd, void* patches, int B, int C, int Hi, int Wi, int p, void* stream),
      px, mean, sd, patches, B, C, Hi, Wi, p, stream)
ENTRY(int, cara_im2col_patches_u8_rows,
      (const unsigned char* px, int n_split, const int64_t* rows, const float* mean, const float* sd, void* patches, int* bad, int B, int C, int Hi, int Wi, int p,
       void* stream),
      px, n_split, rows, mean, sd, patches, bad, B, C, Hi, Wi, p, stream)
ENTRY(int, cara_im2col_patches_u8_rows_crop,
      (const unsigned char* px, int n_split, int Hs, int Ws, const int64_t* rows, const int* boxes, const float* mean, const float* sd, void* patches, int* bad,
       int B, int C, int Hi, int Wi, int p, void* stream),
      px, n_split, Hs, Ws, rows, boxes, mean, sd, patches, bad, B, C, Hi, Wi, p, stream)
ENTRY(int, cara_gemm_bf16, (const cara_gemm_args* a, void* stream), a, stream)
ENTRY(int, cara_assemble_tokens, (const float* emb, const float* cls, const float* pos, float* x, int B, int P, int D, void* stream), emb, cls, pos, x, B, P, D, stream)
ENTRY(int, cara_layernorm_fwd_ex,
      (const float* x, long ldx, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int M, int C, float eps, const void* Ut, int rank, int Rp,
       void* T, void* Tt, int ldt, int y_panels, void* stream),
      x, ldx, gamma, beta, y, mean, rstd, M, C, eps, Ut, rank, Rp, T, Tt, ldt, y_panels, stream)
ENTRY(int, cara_layernorm_bwd,
      (const void* dy, const float* x, long ldx, const float* gamma, const float* mean, const float* rstd, const float* dx_in, float* dx_out, void* dyb,
       const float* rowscale, int rows_per_sample, int M, int C, void* stream),
      dy, x, ldx, gamma, mean, rstd, dx_in, dx_out, dyb, rowscale, rows_per_sample, M, C, stream)
ENTRY(int, cara_layernorm_bwd_ex,
      (const void* dy, const float* x, long ldx, const float* gamma, const float* mean, const float* rstd, const float* dx_in, float* dx_out, void* dyb,
       const float* rowscale, int rows_per_sample, int M, int C, const void* Vst, int rank, int Rp, void* G, void* Gt, int ldt, int dyb_panels, void* stream),
      dy, x, ldx, gamma, mean, rstd, dx_in, dx_out, dyb, rowscale, rows_per_sample, M, C, Vst, rank, Rp, G, Gt, ldt, dyb_panels, stream)
ENTRY(int, cara_token_mean, (const float* x, int B, int tokens, int first, int D, float* out, void* stream), x, B, tokens, first, D, out, stream)
ENTRY(int, cara_token_mean_bwd,
      (const float* dpool, const float* rowscale, int B, int tokens, int first, int D, float* dx, void* dyb, int dyb_panels, void* stream),
      dpool, rowscale, B, tokens, first, D, dx, dyb, dyb_panels, stream)
ENTRY(int, cara_attention_fwd, (const void* qkv, void* out, float* lse, int B, int N, int H, float scale, void* stream), qkv, out, lse, B, N, H, scale, stream)
ENTRY(int, cara_attention_cls_fwd, (const void* qkv, void* out, float* lse, int B, int N, int H, float scale, void* stream), qkv, out, lse, B, N, H, scale, stream)
ENTRY(int, cara_attention_bwd, (const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B, int N, int H, float scale, void* stream),
      qkv, out, dout, lse, dqkv, B, N, H, scale, stream)
ENTRY(int, cara_attention_cls_bwd, (const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B, int N, int H, float scale, void* stream),
      qkv, out, dout, lse, dqkv, B, N, H, scale, stream)
ENTRY(int, cara_skinny_xu_r, (const void* X, int ldx, const void* Ut, void* T, void* Tt, int ldt, int M, int K, int Rp, int rank, void* stream),
      X, ldx, Ut, T, Tt, ldt, M, K, Rp, rank, stream)
ENTRY(int, cara_gemm_with_tskinny_r,
      (const cara_gemm_args* a, const void* Xa, int ldxa, const void* Gta, void* slabs_a, int K1a, const void* Xb, int ldxb, const void* Gtb, void* slabs_b, int K1b,
       int colsum_b, int ldg, int M, int Rp, int rank, void* stream),
      a, Xa, ldxa, Gta, slabs_a, K1a, Xb, ldxb, Gtb, slabs_b, K1b, colsum_b, ldg, M, Rp, rank, stream)
ENTRY(int, cara_tskinny_partial2_r,
      (const void* Xa, int ldxa, const void* Gta, void* slabs_a, int K1a, const void* Xb, int ldxb, const void* Gtb, void* slabs_b, int K1b, int colsum_b, int ldg,
       int M, int Rp, int rank, void* stream),
      Xa, ldxa, Gta, slabs_a, K1a, Xb, ldxb, Gtb, slabs_b, K1b, colsum_b, ldg, M, Rp, rank, stream)
ENTRY(int, cara_tskinny_partial2_small,
      (const void* Xa, int ldxa, const void* Gta, void* slabs_a, int K1a, const void* Xb, int ldxb, const void* Gtb, void* slabs_b, int K1b, int colsum_b, int ldg,
       int M, int Rp, int rank, void* stream),
      Xa, ldxa, Gta, slabs_a, K1a, Xb, ldxb, Gtb, slabs_b, K1b, colsum_b, ldg, M, Rp, rank, stream)
int cara_tskinny_reduce_many(const cara_ts_reduce* p, int n, void* stream) {
  printf("  cara_tskinny_reduce_many( n %d stream %p )\n", n, stream);
  for (int i = 0; i < n; ++i) {   // (field by field: the entries are built member-wise, their padding is not defined)
    printf("    entry %d: slabs %p stride %zu D %p colsum %p batch %d M %d K1 %d Rp %d Rc %d wave_slabs %d\n", i, p[i].slabs, p[i].slab_stride,
           (const void*)p[i].D, (const void*)p[i].colsum, p[i].batch, p[i].M, p[i].K1, p[i].Rp, p[i].Rc, p[i].wave_slabs);
  }
  return leave("cara_tskinny_reduce_many", REAL(cara_tskinny_reduce_many)(p, n, stream));
}
ENTRY(int, cara_gemm_rider_slab_format, (const cara_gemm_args* a, int Rp, int rank), a, Rp, rank)
ENTRY(int, cara_gemm_dv_chunks, (const cara_gemm_args* a, int riders), a, riders)
ENTRY(int, cara_gemm_epi_rider_chunks, (const cara_gemm_args* a), a)
ENTRY(int, cara_factor_grad_reduce_ex,
      (const cara_geom* g, const cara_cp* cp, const cara_layer_grads* lg, const cara_cp* grads, void* scratch, const float* loss_scale, float* found_inf, void* stream),
      g, cp, lg, grads, scratch, loss_scale, found_inf, stream)
ENTRY(int, cara_dense_delta_grad, (const cara_geom* g, const cara_cp* cp, const float* dD, const cara_cp* grads, void* scratch, void* stream),
      g, cp, dD, grads, scratch, stream)
ENTRY(int, cara_materialize_merge,
      (const void* W, const void* U, const void* Vs, int Rp, int out, int in, float p, unsigned seed, unsigned id, void* Weff, void* stream),
      W, U, Vs, Rp, out, in, p, seed, id, Weff, stream)
ENTRY(int, cara_transpose_bf16_ld, (const void* src, long lds, void* dst, long ldd, int rows, int cols, void* stream), src, lds, dst, ldd, rows, cols, stream)
ENTRY(int, cara_colsum_bf16, (const void* X, int ld, int M, int N, float* out, void* scratch, void* stream), X, ld, M, N, out, scratch, stream)
ENTRY(int, cara_gemm_tn_f32,
      (const void* At, int lda, const void* Bt, int ldb, float* C, int ldc, int M, int N, int K, int nslab, size_t slab_stride, void* stream),
      At, lda, Bt, ldb, C, ldc, M, N, K, nslab, slab_stride, stream)
ENTRY(int, cara_sum_slabs_f32, (const float* slabs, int nslab, size_t slab_stride, size_t count, float* out, void* stream), slabs, nslab, slab_stride, count, out, stream)
ENTRY(int, cara_dropout_grad_contract,
      (const float* dW, int nslab, size_t slab_stride, const void* U, const void* Vs, int Rp, int out, int in, float p, unsigned seed, unsigned id, float* dU, float* dVs,
       void* scratch, void* stream),
      dW, nslab, slab_stride, U, Vs, Rp, out, in, p, seed, id, dU, dVs, scratch, stream)
}
// (library-internal, C++ linkage: declared in the library's common.h)
int cara_layernorm_bwd_rows_in(const void* dy, const float* x, long ldx, const float* gamma, const float* mean, const float* rstd, const float* dx_in, float* dx_out,
                               void* dyb, const float* rowscale, int rows_per_sample, int M, int C, const void* Vst, int rank, int Rp, void* G, void* Gt, int ldt,
                               int dyb_panels, int dx_in_every, void* stream) {
  enter("cara_layernorm_bwd_rows_in", dy, x, ldx, gamma, mean, rstd, dx_in, dx_out, dyb, rowscale, rows_per_sample, M, C, Vst, rank, Rp, G, Gt, ldt, dyb_panels,
        dx_in_every, stream);
  typedef decltype(&cara_layernorm_bwd_rows_in) Fn;
  Dl_info self;   // (the mangled name is this definition's own)
  Fn real = dladdr(reinterpret_cast<void*>(&cara_layernorm_bwd_rows_in), &self) && self.dli_sname ? reinterpret_cast<Fn>(dlsym(RTLD_NEXT, self.dli_sname)) : nullptr;
  if (!real) { fprintf(stderr, "host_trace: cara_layernorm_bwd_rows_in not found in the library\n"); exit(2); }
  return leave("cara_layernorm_bwd_rows_in", real(dy, x, ldx, gamma, mean, rstd, dx_in, dx_out, dyb, rowscale, rows_per_sample, M, C, Vst, rank, Rp, G, Gt, ldt,
                                                  dyb_panels, dx_in_every, stream));
}

// ---- the cases ----
namespace {
struct Shape { const char* what; int depth, dim, rank, Rp, B, img, order, exact; };
// (the two shapes of test_backward_schedule_regimes_with_a_middle_block; the headline shape; ranks; a small batch; cls-rows-only last
// blocks that carry products (1104 rows) and flush a dU with other rows (1100); tensorisation orders; exact weight dropout; depth 1)
const Shape SHAPES[] = {
    {"depth 3, 96 px, batch 28 (M = 1036)", 3, 768, 16, 32, 28, 96, 4, 0},
    {"depth 3, 96 px, batch 112 (M = 4144)", 3, 768, 16, 32, 112, 96, 4, 0},
    {"depth 12, 224 px, batch 64", 12, 768, 16, 32, 64, 224, 4, 0},
    {"rank 5", 2, 768, 5, 32, 64, 224, 4, 0},
    {"rank 8", 2, 768, 8, 32, 64, 224, 4, 0},
    {"rank 32", 2, 768, 32, 32, 64, 224, 4, 0},
    {"rank 48", 2, 768, 48, 64, 64, 224, 4, 0},
    {"rank 64", 2, 768, 64, 64, 64, 224, 4, 0},
    {"batch 4", 2, 768, 16, 32, 4, 224, 4, 0},
    {"cls rows 1104", 2, 768, 16, 32, 1104, 32, 4, 0},
    {"cls rows 1100", 2, 768, 16, 32, 1100, 32, 4, 0},
    {"order 2", 2, 768, 16, 32, 32, 224, 2, 0},
    {"order 3", 2, 768, 16, 32, 32, 224, 3, 0},
    {"order 5", 2, 768, 16, 32, 32, 224, 5, 0},
    {"exact weight dropout", 2, 768, 16, 32, 32, 224, 4, 1},
    {"depth 1", 1, 768, 16, 32, 64, 224, 4, 0},
};
// HOST_TRACE_POOL=1: the mean-pooled readout (the last block on all its rows, the pool and its backward in the memsets' place), at the
// regimes above that differ in the last block; with exact weight dropout both entries refuse
const Shape POOLED[] = {
    {"pooled, depth 3, 96 px, batch 28 (M = 1036)", 3, 768, 16, 32, 28, 96, 4, 0},
    {"pooled, depth 12, 224 px, batch 64", 12, 768, 16, 32, 64, 224, 4, 0},
    {"pooled, rank 64", 2, 768, 64, 64, 64, 224, 4, 0},
    {"pooled, batch 4", 2, 768, 16, 32, 4, 224, 4, 0},
    {"pooled, order 2", 2, 768, 16, 32, 32, 224, 2, 0},
    {"pooled, exact weight dropout (refused)", 2, 768, 16, 32, 32, 224, 4, 1},
    {"pooled, depth 1", 1, 768, 16, 32, 64, 224, 4, 0},
};

template <class T>
T* fake(int i) { return reinterpret_cast<T*>((uintptr_t)0x100000000000ull + (uintptr_t)i * 0x1000000000ull); }
}  // namespace

int main() {
  if (getenv("HOST_TRACE_SITES")) printf("cara_profile_sites -> %d\n", cara_profile_sites(~0ull, 1));
  void* stream = reinterpret_cast<void*>(0x5700);
  void* ws = reinterpret_cast<void*>(0x700000000000ull);
  int n = 0;
  cara_vit_weights w = {};
  w.patch_w = fake<void>(n++); w.patch_b = fake<float>(n++); w.cls = fake<float>(n++); w.pos = fake<float>(n++);
  w.ln1_g = fake<float>(n++); w.ln1_b = fake<float>(n++); w.ln2_g = fake<float>(n++); w.ln2_b = fake<float>(n++);
  w.qkv_w = fake<void>(n++); w.qkv_wt = fake<void>(n++); w.qkv_b = fake<float>(n++);
  w.proj_w = fake<void>(n++); w.proj_wt = fake<void>(n++); w.proj_b = fake<float>(n++);
  w.fc1_w = fake<void>(n++); w.fc1_wt = fake<void>(n++); w.fc1_b = fake<float>(n++);
  w.fc2_w = fake<void>(n++); w.fc2_wt = fake<void>(n++); w.fc2_b = fake<float>(n++);
  w.norm_g = fake<float>(n++); w.norm_b = fake<float>(n++);
  w.qkv_wp = fake<void>(n++); w.qkv_wtp = fake<void>(n++); w.proj_wp = fake<void>(n++); w.proj_wtp = fake<void>(n++);
  w.fc1_wp = fake<void>(n++); w.fc1_wtp = fake<void>(n++); w.fc2_wp = fake<void>(n++); w.fc2_wtp = fake<void>(n++);
  cara_cp cp, grads;
  float** c = reinterpret_cast<float**>(&cp);
  float** gr = reinterpret_cast<float**>(&grads);
  for (int i = 0; i < 13; ++i) { c[i] = fake<float>(n++); gr[i] = fake<float>(n++); }
  const float *head_w = fake<float>(n++), *head_b = fake<float>(n++), *droppath = fake<float>(n++), *dlogits = fake<float>(n++);
  float *logits = fake<float>(n++), *dhead_w = fake<float>(n++), *dhead_b = fake<float>(n++);
  const float *images = fake<float>(n++), *mean = fake<float>(n++), *stdv = fake<float>(n++);
  const unsigned char* pixels = fake<unsigned char>(n++);
  const int64_t* rows = fake<int64_t>(n++);
  const int* boxes = fake<int>(n++);
  int* bad = fake<int>(n++);

  const bool pooled = getenv("HOST_TRACE_POOL") != nullptr;
  const Shape* shapes = pooled ? POOLED : SHAPES;
  const size_t nshapes = pooled ? sizeof(POOLED) / sizeof(POOLED[0]) : sizeof(SHAPES) / sizeof(SHAPES[0]);
  for (size_t i = 0; i < nshapes; ++i) {
    const Shape& sh = shapes[i];
    cara_geom g = {sh.depth, sh.dim, sh.dim / 64, sh.rank, sh.Rp, 0.1f, sh.order};
    cara_vit_shape s = {};
    s.pool = pooled ? 1 : 0;
    s.B = sh.B; s.img = sh.img; s.patch = 16; s.chans = 3; s.tokens = (sh.img / 16) * (sh.img / 16) + 1; s.num_classes = 100;
    s.eps = 1e-6f; s.wd_exact = sh.exact; s.wd_p = 0.1f; s.wd_seed = 1234u;
    printf("==== %s: depth %d dim %d rank %d Rp %d B %d img %d order %d exact %d\n", sh.what, sh.depth, sh.dim, sh.rank, sh.Rp, sh.B, sh.img, sh.order, sh.exact);
    for (int inference = 0; inference < 2; ++inference) {
      s.inference = inference;
      printf("== inference %d: cara_vit_workspace_bytes -> %zu\n", inference, cara_vit_workspace_bytes(&g, &s));
      printf("== cara_vit_forward\n");
      printf("== -> %d\n", cara_vit_forward(&g, &s, &w, &cp, head_w, head_b, images, droppath, ws, logits, stream));
      printf("== cara_vit_forward_u8\n");
      printf("== -> %d\n", cara_vit_forward_u8(&g, &s, &w, &cp, head_w, head_b, pixels, mean, stdv, droppath, ws, logits, stream));
      printf("== cara_vit_forward_u8_rows\n");
      printf("== -> %d\n", cara_vit_forward_u8_rows(&g, &s, &w, &cp, head_w, head_b, pixels, 50000, rows, mean, stdv, droppath, ws, logits, bad, stream));
      printf("== cara_vit_forward_u8_rows_crop\n");
      printf("== -> %d\n", cara_vit_forward_u8_rows_crop(&g, &s, &w, &cp, head_w, head_b, pixels, 50000, sh.img + 32, sh.img + 16, rows, boxes, mean, stdv, droppath,
                                                         ws, logits, bad, stream));
      printf("== cara_vit_backward\n");
      printf("== -> %d\n", cara_vit_backward(&g, &s, &w, &cp, head_w, dlogits, droppath, ws, &grads, dhead_w, dhead_b, stream));
    }
  }
  return 0;
}
