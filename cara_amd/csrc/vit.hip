// Whole adapted ViT forward / backward as stream-ordered sequences of the kernels in this
// library (gfx950).  What `model(x)` and `loss.backward()` of
// /root/reference/image_classification/vit_cp.py:46-49 execute, with the patched forwards of
// /root/reference/src/cara/cara.py:15-95 in factored form: no dW is ever
// materialised and no dense weight gradient exists; the frozen backbone only propagates dX.
// Host side is plain C++ in the library so a train step costs two FFI calls and the whole
// sequence can be captured in a hipGraph (nothing here allocates or synchronises).
#include <stdlib.h>

#include <mutex>

#include "common.h"
#include "gemm8.h"

namespace {

struct Carver {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off = (off + bytes + 255) & ~(size_t)255;
    return o;
  }
};

struct LayerWs {
  size_t x_in, x_mid, mean1, rstd1, mean2, rstd2;
  size_t xn1, qkv, lse, ao, xn2, u, h;
  size_t T[4], Tt[4];   // qkv, proj, fc1, fc2
};

struct Ws {
  size_t pack, patches, emb, head_wb, clsn, meanF, rstdF, x_last;
  bool pool;                // cara_vit_shape::pool = 1: the mean-pooled readout
  size_t pooled, dpooled;   // ... then only: the mean of the patch rows of x_last [B, D] fp32, and its gradient
  LayerWs layer[64];
  // backward
  size_t dx, dXn, dAO, dclsn, gscratch, gemm_scratch;
  // dY of the four linears, G' = dY Vs and its transpose: one set, reused by every block (everything runs in
  // stream order on the caller's stream)
  struct Bwd { size_t dyb_fc2, dyb_proj, dH, dQKV, G[4], Gt[4]; } bwd;
  size_t dU[4], dVs[4], dc[4];
  size_t slabU[4], slabV[4], strideU[4], strideV[4];   // per linear: depth regions of tskinny slabs
  // exact weight-dropout mode: merged weights of every layer (and their transposes), transposed activations, dense dW
  size_t weff[4], wefft[4], dYt, Xt, dWd, xscratch;
  // order-2 QKV tensorisation (cara_geom::cp_length == 2): the dense deltas of every layer and their transposes, the dense
  // dD = x^T dY_k of every (layer, projection), split-K slabs of one such product, scratch of cara_dense_delta_grad
  size_t dd, ddt, dD, dd_slabs, dd_scratch;
  int nslab;   // split-K slabs of the dense dW product
  int ldk;   // row stride of the transposed activations: M rounded up to the GEMM's K granule
  size_t total;
  int M, ldt;
};

size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

// split-K slabs of the dense dW = dY^T X of one linear (cara_gemm_tn_f32): enough of them that (out / 128)(in / 128) tiles
// times slabs fill the chip (proj: 36 tiles -- at four slabs each workgroup walked 98 K steps on a quarter of the CUs:
// 73 us for 15 GF), at least 512 token rows per slab, at most 16
int dw_slabs(int out, int in, int M) {
  const int tiles = ((out + 127) / 128) * ((in + 127) / 128);
  int n = (640 + tiles - 1) / tiles;
  n = n > 16 ? 16 : n;
  while (n > 1 && M / n < 512) --n;
  return n < 1 ? 1 : n;
}

// A/B switches, read ONCE per process (tools/ab_env.sh); the defaults are what DESIGN.md reports.
int env_once(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// The placements of the backward's products that need slab regions of their own size, as far as the shape and the switches allow them
// at all (the block plan below): layout() sizes the regions for them, plan_block() chooses among them per block.  epilogue
// (CARA_EPI_RIDERS): fc2's dU and fc1's dVs out of the fc2 dX epilogue; a_tiles (CARA_DV): fc1's / qkv's dVs out of their dX tiles.
struct Placements { bool epilogue, a_tiles; };
Placements placements(const cara_geom* g, const cara_vit_shape* s, int rows);

bool layout(const cara_geom* g, const cara_vit_shape* s, Ws* w) {
  if (!g || !s || g->depth <= 0 || g->depth > 64 || g->dim % g->heads || g->dim / g->heads != 64) return false;
  if (!(g->Rp == 32 || g->Rp == 64) || g->rank > g->Rp || s->B <= 0 || s->tokens <= 1) return false;
  // (no token limit of the kernels' own: attention streams K / V above 608 tokens; row counts and row indices are int)
  if (s->tokens > (1 << 20) || (long long)s->B * s->tokens >= (1ll << 31)) return false;
  // (a patch dropout runs the blocks on 1 + K of the grid's tokens, 1 <= K <= grid: every per-token region below is sized by
  // `tokens`; which entries take fewer tokens than the grid has is theirs to say, vit_forward_body)
  if (s->img % s->patch || s->tokens > (s->img / s->patch) * (s->img / s->patch) + 1) return false;
  if ((s->chans * s->patch * s->patch) % 64 || g->dim % 256) return false;
  if (!(s->pool == 0 || s->pool == 1) || (s->pool && s->wd_exact)) return false;   // (the pooled readout: not with exact weight dropout)
  const size_t D = g->dim, M = (size_t)s->B * s->tokens, Rp = g->Rp;
  const size_t ldt = (M + 31) / 32 * 32;
  w->M = (int)M;
  w->ldt = (int)ldt;
  Carver c;
  cara_pack_layout pl;
  if (cara_pack_offsets(g, &pl) != CARA_OK) return false;
  w->pack = c.take(pl.total);
  const size_t P = s->tokens - 1, kp = (size_t)s->chans * s->patch * s->patch;
  w->patches = c.take((size_t)s->B * P * kp * 2);
  w->emb = c.take((size_t)s->B * P * D * 4);
  w->head_wb = c.take((size_t)s->num_classes * D * 2);
  w->clsn = c.take((size_t)s->B * D * 2);
  w->meanF = c.take((size_t)s->B * 4);
  w->rstdF = c.take((size_t)s->B * 4);
  // Everything a forward needs besides the blocks' activations comes first, so that the layout of a forward that no
  // backward follows (below) is a PREFIX of the training layout: scratch of the few-row split-K products (partial
  // products, written before they are read) and, for the order-2 tensorisation, the dense QKV deltas and their transposes.
  w->gemm_scratch = c.take(cara_gemm_scratch_bytes());
  w->dd = w->ddt = w->dD = w->dd_slabs = w->dd_scratch = 0;
  if (g->cp_length == 2) {
    if (s->wd_exact) return false;   // (the dense-delta QKV form and the exact weight-dropout mode are not combined)
    if (g->dim % 128) return false;  // (its backward's dense x^T dY: 128 x 128 output tiles, cara_gemm_tn_f32)
    w->dd = c.take((size_t)g->depth * 3 * D * D * 2);
    w->ddt = c.take((size_t)g->depth * 3 * D * D * 2);
  }
  w->x_last = c.take(M * D * 4);
  // (the pooled readout's rows, only where it is asked for: with pool = 0 no offset and no size moves)
  w->pool = s->pool == 1;
  w->pooled = w->dpooled = 0;
  if (w->pool) w->pooled = c.take((size_t)s->B * D * 4);
  // cara_vit_shape::inference (as cara_vit_forward reads it: never with the exact weight-dropout mode): two activation
  // sets, which the blocks take in turn -- block l reads the residual stream from set l % 2 and leaves it in the other
  // set's x_in -- and nothing of the backward: no gradient stream, no dY / G' set, no slabs, no dense gradients.  Being a
  // prefix of the training layout, the same forward runs on a workspace of either size, whatever a training step left
  // in it, and every kernel sees the launch it sees on the training layout: different addresses only.
  const bool inference = s->inference != 0 && !s->wd_exact;
  const int nsets = inference && g->depth > 2 ? 2 : g->depth;
  for (int l = 0; l < nsets; ++l) {
    LayerWs& L = w->layer[l];
    L.x_in = c.take(M * D * 4);
    L.x_mid = c.take(M * D * 4);
    L.mean1 = c.take(M * 4); L.rstd1 = c.take(M * 4); L.mean2 = c.take(M * 4); L.rstd2 = c.take(M * 4);
    L.xn1 = c.take(M * D * 2);
    L.qkv = c.take(M * 3 * D * 2);
    L.lse = c.take((size_t)s->B * g->heads * s->tokens * 4);
    L.ao = c.take(M * D * 2);
    L.xn2 = c.take(M * D * 2);
    L.u = c.take(M * 4 * D * 2);
    L.h = c.take(M * 4 * D * 2);
    for (int i = 0; i < 4; ++i) {
      L.T[i] = c.take(M * Rp * 2);
      L.Tt[i] = c.take(Rp * ldt * 2);
    }
  }
  for (int l = nsets; l < g->depth; ++l) w->layer[l] = w->layer[l - 2];
  if (inference) {
    w->dx = w->dXn = w->dAO = w->dclsn = w->gscratch = 0;
    w->bwd = Ws::Bwd{};
    w->ldk = (int)((M + 63) / 64 * 64);
    w->nslab = 1;
    w->total = c.off;
    return true;
  }
  w->dx = c.take(M * D * 4);
  w->dXn = c.take(M * D * 2);
  w->dAO = c.take(M * D * 2);
  {
    Ws::Bwd& R = w->bwd;
    R.dyb_fc2 = c.take(M * D * 2);
    R.dyb_proj = c.take(M * D * 2);
    R.dH = c.take(M * 4 * D * 2);
    R.dQKV = c.take(M * 3 * D * 2);
    for (int i = 0; i < 4; ++i) {
      R.G[i] = c.take(M * Rp * 2);
      R.Gt[i] = c.take(Rp * ldt * 2);
    }
  }
  w->dclsn = c.take((size_t)s->B * D * 2);
  if (w->pool) w->dpooled = c.take((size_t)s->B * D * 4);
  w->gscratch = c.take(cara_factor_grad_scratch_bytes(g));
  const size_t ins[4] = {D, D, D, 4 * D}, outs[4] = {3 * D, D, 4 * D, D};
  const Placements can = placements(g, s, (int)M);
  for (int i = 0; i < 4; ++i) {
    w->dU[i] = c.take((size_t)g->depth * ins[i] * Rp * 4);
    w->dVs[i] = c.take((size_t)g->depth * outs[i] * Rp * 4);
    w->dc[i] = c.take((size_t)g->depth * outs[i] * 4);
    w->strideU[i] = (cara_tskinny_scratch_bytes((int)M, (int)ins[i], (int)Rp) + 255) & ~(size_t)255;
    w->strideV[i] = (cara_tskinny_scratch_bytes((int)M, (int)outs[i], (int)Rp) + 255) & ~(size_t)255;
    // fc2's dU and fc1's dVs may come out of the fc2 dX epilogue, one slab per 160-row tile (cara_gemm_args::er_*)
    const size_t er_bytes = (cara_gemm_epi_rider_scratch_bytes((int)((M + 127) / 128), (int)(4 * D)) + 255) & ~(size_t)255;   // (row tiles of 128 or 160)
    if (i == 3 && can.epilogue && er_bytes > w->strideU[i]) w->strideU[i] = er_bytes;
    if (i == 2 && can.epilogue && er_bytes > w->strideV[i]) w->strideV[i] = er_bytes;
    // (CARA_DV: fc1's / qkv's dVs out of their dX tiles, one slab per 160-row tile and K step: K1 = the linear's out features)
    const size_t dv_bytes = (cara_gemm_epi_rider_scratch_bytes((int)((M + 159) / 160), (int)outs[i]) + 255) & ~(size_t)255;
    if ((i == 0 || i == 2) && can.a_tiles && dv_bytes > w->strideV[i]) w->strideV[i] = dv_bytes;
    w->slabU[i] = c.take(w->strideU[i] * g->depth);
    w->slabV[i] = c.take(w->strideV[i] * g->depth);
  }
  w->ldk = (int)((M + 63) / 64 * 64);
  w->nslab = 1;
  if (s->wd_exact) {
    // dW = dY^T X has only (out/128) x (in/128) = 36..144 output tiles: its K = M is cut into equal slabs (one
    // batched launch fills the chip), which cara_dropout_grad_contract sums
    w->nslab = M >= 8192 ? 4 : (M >= 3072 ? 2 : 1);
    w->ldk = (int)((M + 64 * w->nslab - 1) / (64 * w->nslab) * (64 * w->nslab));
    for (int i = 0; i < 4; ++i) {
      w->weff[i] = c.take((size_t)g->depth * outs[i] * ins[i] * 2);
      w->wefft[i] = c.take((size_t)g->depth * outs[i] * ins[i] * 2);
    }
    w->dYt = c.take((size_t)4 * D * w->ldk * 2);
    w->Xt = c.take((size_t)4 * D * w->ldk * 2);
    size_t dwd = (size_t)w->nslab * 4 * D * D * 4;   // the transposed-copies route: nslab slabs of the largest product
    for (int i = 0; i < 4; ++i) dwd = max_sz(dwd, (size_t)dw_slabs((int)outs[i], (int)ins[i], (int)M) * outs[i] * ins[i] * 4);
    w->dWd = c.take(dwd);
    w->xscratch = c.take(max_sz(cara_dropout_grad_scratch_bytes((int)(4 * D), (int)D, (int)Rp), cara_colsum_scratch_bytes((int)(4 * D))));
  }
  if (g->cp_length == 2) {
    w->dD = c.take((size_t)g->depth * 3 * D * D * 4);
    w->dd_slabs = c.take((size_t)dw_slabs((int)D, (int)D, (int)M) * D * D * 4);
    w->dd_scratch = c.take(cara_dense_delta_grad_scratch_bytes(g));
  }
  w->total = c.off;
  return true;
}

#define TRY(expr)                 \
  do {                            \
    const int _st = (expr);       \
    if (_st != CARA_OK) return _st; \
  } while (0)

// Optional HIP-event brackets around the kernels of chosen call sites (cara_profile_sites), so that bench.py can
// report average launch durations from INSIDE its timed region, on the stream the kernels run on.  Diagnostic
// state, process-global, off by default; every bracket idles the chip ~15 us (three event records).
struct Prof {
  unsigned long long mask = 0;
  int every = 1;   // bracket the layers l with l % every == 0
  bool made = false;
  long n[CARA_SITE_COUNT] = {};
  hipEvent_t ev[CARA_SITE_COUNT][CARA_SITE_RING][3];
};
Prof g_prof;

// How a linear's transposed skinny products left their partial sums, per layer: 0 = one slab per block, 1 = one per wave
// (cara_gemm_rider_slab_format: the launches of the 160 x 256 x 64 tile stream their riding products with helper waves).
// The end-of-pass reduction groups the layers of a linear by it.
struct SlabFormats {
  unsigned short U[4][64] = {}, V[4][64] = {};   // (>= 2: that many slabs per column block, cara_ts_reduce::wave_slabs)
};

// One transposed skinny product of the backward -- a linear's dU = X^T G' or its dVs = dY^T T (+ dc = colsum dY) -- as
// cara_tskinny_partial2_r / cara_gemm_with_tskinny_r take it.  X == nullptr: none.
struct Product {
  const void* X = nullptr;   // [M, K1], row stride ldx (ldx < 0: K-panel-major with -ldx rows per panel)
  int ldx = 0;
  const void* Gt = nullptr;  // the skinny operand, transposed (G'^T or T^T)
  void* slabs = nullptr;     // its partial sums, this layer's region
  int K1 = 0, colsum = 0, M = 0;
  unsigned short* format = nullptr;   // its cell of SlabFormats: written by whatever launch computes the product
};

// Where the two products of a linear are computed (plan_block decides, once per block; lin_bwd has one arm per value)
enum class Riders {
  Own,        // dVs (+ dc) behind the tiles of the linear's own dX launch, dU behind those of the NEXT dX launch of the pass
  Epilogue,   // fc2 under CARA_EPI_RIDERS: the epilogue of its dX launch computes its dU and fc1's dVs (+ dc)
  DoneAbove,  // fc1 after such a launch: a plain dX GEMM, only its dU waits
  ATiles,     // CARA_DV: dVs (+ dc) out of the A tiles of the linear's own dX launch on the 160 x 256 x 64 tile
  BothHome,   // fc2 beside an ATiles fc1: both its products behind its own tiles; the dU that waits rides behind fc1's (19 MB, not fc2's 77)
  Side,       // CARA_FC1_SIDE: fc1's dVs (+ dc) and the waiting dU as a launch on the side stream under fc1's dX GEMM
};

// CARA_FC1_SIDE=1 (default 0): the two heavy riders of the backward -- fc1's dVs = dH^T T (+ dc) and fc2's dU = h^T G', 154 MB -- as a
// launch of their own on a SIDE stream under the fc1 dX GEMM, which then runs on the 160 x 256 x 64 tile (one workgroup per CU: the
// products' blocks, 40 KiB of LDS and one wave per SIMD each, fit beside it).  One event record on the caller's stream per block
// (the fork); the join is a wait on an event that completed long before.  The stream and the two events are created once per process.
struct SideStream {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  bool ok = false;
};
SideStream* side_stream() {
  // one stream + event pair per DEVICE, created under a lock on first use there (a process-wide pair made on
  // whichever device was current at first use belongs to the wrong device in a multi-device or multi-threaded process)
  static SideStream per_dev[16];
  static bool tried[16] = {};
  static std::mutex mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  SideStream& s = per_dev[dev];
  if (!tried[dev]) {
    tried[dev] = true;
    s.ok = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) == hipSuccess &&
           hipEventCreateWithFlags(&s.fork, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&s.join, hipEventDisableTiming) == hipSuccess;
  }
  return s.ok ? &s : nullptr;
}
// What a backward pass carries from one launch to the next
struct BwdPass {
  Product waiting;            // the dU of the linear before, until the next dX launch carries it (flush_waiting runs it alone otherwise)
  SlabFormats formats;
  bool epilogue_ran = false;  // this block's fc2 dX launch took the Epilogue placement (it falls back to Own where the launch says no)
  bool side_join = false;     // the side stream holds work the caller's stream has not waited for
};

// A 16-bit activation of the workspace and how it lies there: row-major with row stride ld, or K-panel-major ([K/32][panels][32],
// cara_gemm_args::a_panels / c_panels) with `panels` rows per panel (0: row-major), as the block plan says (made by Ctx::act).
struct Act {
  bf16* p;
  int ld, panels;
  int stride() const { return panels ? -panels : ld; }   // the signed stride of the C ABI (cara_skinny_xu_r, Product::ldx)
};
// ... as the A operand of a GEMM / as its 16-bit output
void reads(cara_gemm_args& a, const Act& x) { a.A = x.p; a.lda = x.panels ? 0 : x.ld; if (x.panels) a.a_panels = x.panels; }
void writes(cara_gemm_args& a, const Act& y) { a.C = y.p; if (y.panels) { a.c_panels = y.panels; a.ldc = y.ld; } }

// per-pass context: what lin_fwd / lin_bwd and their exact / dense variants need besides their operands (nothing here outlives the
// call).  The first group is set once per pass, the second once per block.
struct Ctx {
  void* stream;
  char* ws;          // the workspace and its layout
  const Ws* W;
  const cara_vit_shape* s;
  int Rp, ldt;
  int rank;          // the adapter's rank (0: unknown, the skinny passes compute all Rp columns)
  BwdPass* bwd = nullptr;
  const LayerWs* lw = nullptr;
  int layer = 0;
  int rows = 0;      // the rows this half of the block runs on: all M token rows, or the cls rows of the last block
  bool full = false; // ... all token rows (site brackets); on(): the pass's context for one half of a block
  Act act(size_t off, int ld, int panels = 0) const { return Act{reinterpret_cast<bf16*>(ws + off), ld, panels}; }
  float* f32(size_t off) const { return reinterpret_cast<float*>(ws + off); }
  Ctx on(const LayerWs& l, int layer_, int rows_, bool full_) const { Ctx c = *this; c.lw = &l; c.layer = layer_; c.rows = rows_; c.full = full_; return c; }
};

// the rank the transposed skinny products are told
inline int ts_rank(const Ctx& cx) { return cx.rank > 0 ? cx.rank : cx.Rp; }

// One or two products as a launch of their own (a lone product takes the launch's second slot).  small: the two-stage-ring form
// that fits beside a GEMM of the 160 x 256 x 64 tile.
int launch_products(const Ctx& cx, const Product* p0, const Product* p1, void* stream, bool small = false) {
  if (!p1) { p1 = p0; p0 = nullptr; }
  const Product none, &a = p0 ? *p0 : none, &b = *p1;
  if (p0) *a.format = 0;
  *b.format = 0;
  return (small ? cara_tskinny_partial2_small : cara_tskinny_partial2_r)(a.X, a.ldx, a.Gt, a.slabs, a.K1, b.X, b.ldx, b.Gt, b.slabs, b.K1, b.colsum, cx.ldt,
                                                                         b.M, cx.Rp, ts_rank(cx), stream);
}

// One dX GEMM launch with zero, one or two products riding behind its tiles (a lone product takes the launch's second slot); the
// launch says how its riders leave their partial sums (it depends on the arguments only)
int gemm_with_riders(const Ctx& cx, const cara_gemm_args& a, const Product* p0, const Product* p1) {
  if (!p1) { p1 = p0; p0 = nullptr; }
  if (!p1) return cara_gemm_bf16(&a, cx.stream);
  const Product none, &r0 = p0 ? *p0 : none, &r1 = *p1;
  const unsigned short f = (unsigned short)cara_gemm_rider_slab_format(&a, cx.Rp, ts_rank(cx));
  if (p0) *r0.format = f;
  *r1.format = f;
  return cara_gemm_with_tskinny_r(&a, r0.X, r0.ldx, r0.Gt, r0.slabs, r0.K1, r1.X, r1.ldx, r1.Gt, r1.slabs, r1.K1, r1.colsum, cx.ldt, a.M, cx.Rp,
                                  ts_rank(cx), cx.stream);
}

// the dU that found no carrier, as a launch of its own
int flush_waiting(const Ctx& cx) {
  Product& q = cx.bwd->waiting;
  if (!q.X) return CARA_OK;
  const Product dU = q;
  q = Product{};
  return launch_products(cx, &dU, nullptr, cx.stream);
}

bool g_inside_enabled(int slot);

struct SiteBracket {   // RAII: event 0 .. kernel(s) .. event 1, event 2 (an empty bracket: the markers' own cost)
  hipEvent_t* ev = nullptr;
  hipStream_t st;
  SiteBracket(int site, const Ctx& cx) : st(static_cast<hipStream_t>(cx.stream)) {
    // (block every / 2 of every run of `every` blocks: never block 0, whose qkv dX and LayerNorm-1 backward do not exist)
    if (!(g_prof.mask >> site & 1ull) || !cx.full || cx.layer % g_prof.every != g_prof.every / 2) return;
    ev = g_prof.ev[site][g_prof.n[site]++ % CARA_SITE_RING];
    (void)hipEventRecord(ev[0], st);
  }
  ~SiteBracket() {
    if (!ev) return;
    (void)hipEventRecord(ev[1], st);
    (void)hipEventRecord(ev[2], st);
  }
};

struct Lin {  // one adapted linear of one layer
  const bf16 *W, *Wt;
  const bf16 *Ut, *U, *Vs, *Vst;
  const float* bias;
  int in, out, slot;
  const bf16 *Wp = nullptr, *Wtp = nullptr;   // K-panel-major images of W / Wt (cara_gemm_args::Bp), or null
};

// CARA_FUSE_GEMM_T bit 0 (default on) computes T = X U of forward proj / fc2 inside the GEMM that consumes it
// (cara_gemm_args::Ut) instead of a separate cara_skinny_xu pass
bool fuse_gemm_t(int Mr, int Rp) {
  static const int v = env_once("CARA_FUSE_GEMM_T", 1);
  return (v & 1) != 0 && (Rp == 32 || Rp == 64) && Mr >= 1024;
}

// CARA_FUSE_TS=0: the transposed skinny products of a linear run as their own launch behind its dX GEMM instead of
// riding in that GEMM's launch (cara_gemm_with_tskinny).  Rp = 32, full-size products only.
bool fuse_ts(int Mr, int Rp) {
  static const int v = env_once("CARA_FUSE_TS", 1);
  return v != 0 && (Rp == 32 || Rp == 64) && Mr >= 1024;
}

void with_scratch(cara_gemm_args& a, const Ctx& cx) {   // split-K scratch of the workspace in use (few-row products)
  a.scratch = cx.ws + cx.W->gemm_scratch;
  a.scratch_bytes = cara_gemm_scratch_bytes();
}

constexpr int SITE_FWD[4] = {CARA_SITE_QKV_FWD, CARA_SITE_PROJ_FWD, CARA_SITE_FC1_FWD, CARA_SITE_FC2_FWD};
constexpr int SITE_BWD[4] = {CARA_SITE_QKV_BWD, CARA_SITE_PROJ_BWD, CARA_SITE_FC1_BWD, CARA_SITE_FC2_BWD};

// forward of one adapted linear on cx.rows rows of X: T = X U ; C = [X | T] [W | Vs]^T + bias -> epilogue (a.ldc == 0: dense output)
// (have_T: the LayerNorm that produced X already left T = X U and its transpose, cara_layernorm_fwd_xu)
int lin_fwd(const Lin& L, const Act& X, cara_gemm_args a, const Ctx& cx, bool have_T = false) {
  void* st = cx.stream;
  const int Mr = cx.rows, Rp = cx.Rp, ldt = cx.ldt;
  bf16* T = cx.act(cx.lw->T[L.slot], Rp).p;
  bf16* Tt = cx.act(cx.lw->Tt[L.slot], ldt).p;
  const bool inside = !have_T && fuse_gemm_t(Mr, Rp);   // T computed by the GEMM itself
  if (!have_T && !inside) {
    SiteBracket b(CARA_SITE_SKINNY_FWD, cx);
    TRY(cara_skinny_xu_r(X.p, X.stride(), L.Ut, T, Tt, ldt, Mr, L.in, Rp, ts_rank(cx), st));
  }
  reads(a, X);
  a.B = L.W; a.Bp = L.Wp; a.ldb = L.in; a.A2 = inside ? nullptr : T; a.B2 = L.Vs; a.Rp = Rp;
  if (inside) {
    static const int t_all = env_once("CARA_GEMM_T_ALL_COLUMNS", 0);   // 1: T inside the GEMM with all Rp columns whatever the rank (A/B runs)
    a.Ut = L.Ut; a.T_out = T; a.Tt_out = Tt; a.ldt = ldt; a.Ut_rank = t_all ? 0 : cx.rank;
  }
  a.M = Mr; a.N = L.out; a.K = L.in; a.bias = L.bias;
  if (a.ldc == 0) a.ldc = L.out;
  with_scratch(a, cx);
  SiteBracket b(SITE_FWD[L.slot], cx);
  return cara_gemm_bf16(&a, st);
}

// backward of one adapted linear given dY (cx.rows rows) and its saved input X:
//   G' = dY Vs ; dX = [dY | G'] [W^T | U]^T (optional) ; dU = X^T G' ; dVs = dY^T T ; dc = colsum dY
// The two transposed skinny products go where `where` says when the dX launch can carry products (fuse_ts); otherwise they are
// one launch of their own behind it, on the same stream.
// (have_G: the LayerNorm backward that produced dY already left G' and its transpose, cara_layernorm_bwd_xu)
int lin_bwd(const Lin& L, const Act& dY, const Act& X, bool want_dx, cara_gemm_args a, bool want_dc, const Ctx& cx, Riders where = Riders::Own,
            bool have_G = false) {
  void* st = cx.stream;
  BwdPass& pass = *cx.bwd;
  char* ws = cx.ws;
  const Ws& W = *cx.W; const LayerWs& lw = *cx.lw;
  const int slot = L.slot, layer = cx.layer, Mr = cx.rows, Rp = cx.Rp, ldt = cx.ldt;
  bf16* G = cx.act(W.bwd.G[slot], Rp).p;
  bf16* Gt = cx.act(W.bwd.Gt[slot], ldt).p;
  const bool carries = want_dx && fuse_ts(Mr, Rp);
  // a dU rides one launch later, so nothing in a linear's own dX launch reads its G': the GEMM computes it on the tiles it streams
  // and the separate pass over dY goes (CARA_GEMM_G_INSIDE=0 keeps the pass)
  const bool g_inside = !have_G && carries && g_inside_enabled(slot) && a.epi == CARA_EPI_BF16;
  if (!have_G && !g_inside) {
    SiteBracket b(CARA_SITE_SKINNY_BWD, cx);
    TRY(cara_skinny_xu_r(dY.p, dY.stride(), L.Vst, G, Gt, ldt, Mr, L.out, Rp, ts_rank(cx), st));
  }
  const Product dU{X.p, X.stride(), Gt, ws + W.slabU[slot] + (size_t)layer * W.strideU[slot], L.in, 0, Mr, &pass.formats.U[slot][layer]};
  const Product dVs{dY.p, dY.stride(), ws + lw.Tt[slot], ws + W.slabV[slot] + (size_t)layer * W.strideV[slot], L.out, want_dc ? 1 : 0, Mr, &pass.formats.V[slot][layer]};
  if (want_dx) {
    reads(a, dY);
    a.B = L.Wt; a.Bp = L.Wtp; a.ldb = L.out; a.A2 = G; a.B2 = L.U; a.Rp = Rp;
    if (g_inside) { a.A2 = nullptr; a.Ut = L.Vst; a.T_out = G; a.Tt_out = Gt; a.ldt = ldt; a.Ut_rank = ts_rank(cx) <= 16 ? ts_rank(cx) : 0; }
    a.M = Mr; a.N = L.in; a.K = L.out; a.bias = nullptr;
    if (a.ldc == 0) a.ldc = L.in;
    with_scratch(a, cx);
  }
  if (!carries) {   // nothing rides (no dX, few rows, CARA_FUSE_TS=0): what waits and this linear's pair run as launches of their own
    if (want_dx) {
      SiteBracket b(SITE_BWD[slot], cx);
      TRY(cara_gemm_bf16(&a, st));
    }
    TRY(flush_waiting(cx));
    return launch_products(cx, &dU, &dVs, st);
  }
  SiteBracket b(SITE_BWD[slot], cx);
  // the dU of the linear before rides here when it has this launch's rows (fc2's, the 77-MB read of h, thus leaves the two-round fc2
  // dX launch for the single-round fc1 dX launch; a dU never shares an operand with its own dX GEMM, so it loses nothing elsewhere)
  if (pass.waiting.X && pass.waiting.M != Mr) TRY(flush_waiting(cx));
  const Product* carried = pass.waiting.X ? &pass.waiting : nullptr;
  // the placements whose products the launch computes itself: one slab per row tile (chunk); Own where the launch or the scratch says no
  int chunks = 0;
  if (where == Riders::ATiles) {
    cara_gemm_args d = a;
    d.er_Tt = dVs.Gt; d.er_ldg = ldt; d.er_slabs_v = dVs.slabs; d.er_colsum = dVs.colsum;
    chunks = cara_gemm_dv_chunks(&d, carried ? 1 : 0);
    if (chunks > 0 && chunks <= 65535 && cara_gemm_epi_rider_scratch_bytes(chunks, L.out) <= W.strideV[slot]) a = d;
    else where = Riders::Own;
  }
  if (where == Riders::Epilogue) {   // (this linear is fc2, X its saved input h; the dVs the epilogue computes is fc1's)
    cara_gemm_args d = a;
    d.er_Tt = ws + lw.Tt[2]; d.er_Gt = Gt; d.er_slabs_v = ws + W.slabV[2] + (size_t)layer * W.strideV[2]; d.er_slabs_u = dU.slabs; d.er_ldg = ldt; d.er_colsum = 1;
    d.er_h = X.p; d.er_h_panels = X.panels;
    chunks = cara_gemm_epi_rider_chunks(&d);
    const size_t room = W.strideV[2] < W.strideU[3] ? W.strideV[2] : W.strideU[3];
    if (chunks > 0 && chunks <= 65535 && cara_gemm_epi_rider_scratch_bytes(chunks, L.in) <= room) a = d;
    else where = Riders::Own;
  }
  switch (where) {
    case Riders::Own:
      TRY(gemm_with_riders(cx, a, carried, &dVs));
      break;
    case Riders::Epilogue:   // (nothing of this linear waits: its dU is in the slabs the epilogue wrote)
      TRY(gemm_with_riders(cx, a, carried, &dVs));
      *dU.format = pass.formats.V[2][layer] = (unsigned short)chunks;   // (fc1's dVs slabs: the same launch, the same count of row tiles)
      pass.epilogue_ran = true;
      pass.waiting = Product{};
      return CARA_OK;
    case Riders::DoneAbove:
      TRY(gemm_with_riders(cx, a, carried, nullptr));
      break;
    case Riders::ATiles:
      TRY(gemm_with_riders(cx, a, carried, nullptr));
      *dVs.format = (unsigned short)chunks;
      break;
    case Riders::BothHome:   // (the dU that waits stays for the next launch)
      return gemm_with_riders(cx, a, &dU, &dVs);
    case Riders::Side: {
      SideStream* ss = side_stream();
      if (!ss) return CARA_E_LAUNCH;
      if (hipEventRecord(ss->fork, static_cast<hipStream_t>(st)) != hipSuccess || hipStreamWaitEvent(ss->stream, ss->fork, 0) != hipSuccess) return CARA_E_LAUNCH;
      TRY(launch_products(cx, carried, &dVs, ss->stream, true));
      if (hipEventRecord(ss->join, ss->stream) != hipSuccess) return CARA_E_LAUNCH;
      pass.side_join = true;
      TRY(cara_gemm_bf16(&a, st));
      break;
    }
  }
  pass.waiting = dU;   // (until the next dX GEMM of the pass)
  return CARA_OK;
}

// ---- order-2 QKV tensorisation: the QKV linear as y = x W^T + x Dm^T with the dense scaled delta Dm (cara_dense_delta_*) ----
int lin_fwd_dense(const Lin& L, const Act& X, cara_gemm_args a, const Ctx& cx) {
  const size_t D = L.in;
  a.A = X.p; a.lda = X.ld; a.B = L.W; a.B3 = cx.act(cx.W->dd, L.in).p + (size_t)cx.layer * 3 * D * D; a.ldb = L.in; a.A2 = nullptr; a.B2 = nullptr; a.Rp = 0;
  a.M = cx.rows; a.N = L.out; a.K = L.in; a.bias = L.bias;
  if (a.ldc == 0) a.ldc = L.out;
  with_scratch(a, cx);
  SiteBracket b(SITE_FWD[L.slot], cx);
  return cara_gemm_bf16(&a, cx.stream);
}
// backward: dX = dY W + dY Dm (optional), and dD[k] = X^T dY_k for the three projections (split-K slabs, summed)
int lin_bwd_dense(const Lin& L, const Act& dYa, const Act& Xa, bool want_dx, cara_gemm_args a, const Ctx& cx) {
  void* st = cx.stream;
  const bf16 *dY = dYa.p, *X = Xa.p;   // (both row-major and dense)
  const int D = L.in, Mr = cx.rows;
  const size_t layer_dd = (size_t)cx.layer * 3 * D * D;   // this layer's three deltas in dd / ddt / dD
  float* dD_l = reinterpret_cast<float*>(cx.ws + cx.W->dD) + layer_dd;
  float* slabs = reinterpret_cast<float*>(cx.ws + cx.W->dd_slabs);
  if (want_dx) {
    a.A = dY; a.lda = L.out; a.B = L.Wt; a.B3 = cx.act(cx.W->ddt, D).p + layer_dd; a.ldb = L.out; a.A2 = nullptr; a.B2 = nullptr; a.Rp = 0;
    a.M = Mr; a.N = L.in; a.K = L.out; a.bias = nullptr;
    if (a.ldc == 0) a.ldc = L.in;
    with_scratch(a, cx);
    SiteBracket b(SITE_BWD[L.slot], cx);
    TRY(cara_gemm_bf16(&a, st));
  }
  const int ns = dw_slabs(D, D, Mr);
  const size_t dd = (size_t)D * D;
  for (int k = 0; k < 3; ++k) {
    TRY(cara_gemm_tn_f32(X, D, dY + (size_t)k * D, L.out, slabs, D, D, D, Mr, ns, dd, st));
    TRY(cara_sum_slabs_f32(slabs, ns, dd, dd, dD_l + (size_t)k * dd, st));
  }
  return CARA_OK;
}

// ---- exact weight-dropout mode (cara_vit_shape::wd_exact): y = x W^T + x (keep/(1-p) dW)^T, two accumulated products ----
// forward of one linear: materialise the masked delta (and its transpose, for dX) of this layer, then C = X (W + Dm)^T + bias
int lin_fwd_exact(const Lin& L, const Act& X, cara_gemm_args a, const Ctx& cx) {
  void* st = cx.stream;
  char* ws = cx.ws;
  const Ws& W = *cx.W; const cara_vit_shape* s = cx.s;
  const int layer = cx.layer, Rp = cx.Rp;
  const size_t wbytes = (size_t)L.out * L.in * 2;
  bf16* weff = reinterpret_cast<bf16*>(ws + W.weff[L.slot] + layer * wbytes);
  bf16* wefft = reinterpret_cast<bf16*>(ws + W.wefft[L.slot] + layer * wbytes);
  // the masked adapter delta on its own (W == NULL), kept apart from the frozen weight: y = x W^T + x Dm^T as two
  // products accumulated in fp32 (cara_gemm_args::B3) -- merged into one bf16 weight, a delta below half an ulp of W
  // would vanish (the reference's zero-initialised A2 / P2: the whole adapter early in training)
  TRY(cara_materialize_merge(nullptr, L.U, L.Vs, Rp, L.out, L.in, s->wd_p, s->wd_seed, (unsigned)(4 * layer + L.slot), weff, st));
  TRY(cara_transpose_bf16_ld(weff, L.in, wefft, L.out, L.out, L.in, st));
  a.A = X.p; a.lda = X.ld; a.B = L.W; a.B3 = weff; a.ldb = L.in; a.A2 = nullptr; a.B2 = nullptr; a.Rp = 0;
  a.M = cx.rows; a.N = L.out; a.K = L.in; a.bias = L.bias;
  if (a.ldc == 0) a.ldc = L.out;
  with_scratch(a, cx);
  return cara_gemm_bf16(&a, st);
}

// backward of one linear: dc = colsum dY; dW = dY^T X (dense, fp32) -> dU, dVs through the regenerated mask;
// dX = dY W_eff (optional).  X and dY are dense [Mr, in] / [Mr, out] (the cls-row shortcut is off in this mode).
int lin_bwd_exact(const Lin& L, const Act& dYa, const Act& Xa, bool want_dx, cara_gemm_args a, bool want_dc, const Ctx& cx) {
  void* st = cx.stream;
  char* ws = cx.ws;
  const Ws& W = *cx.W; const cara_vit_shape* s = cx.s;
  const bf16 *dY = dYa.p, *X = Xa.p;
  const int layer = cx.layer, Mr = cx.rows, Rp = cx.Rp;
  hipStream_t hs = static_cast<hipStream_t>(st);
  const size_t wbytes = (size_t)L.out * L.in * 2;
  bf16* wefft = reinterpret_cast<bf16*>(ws + W.wefft[L.slot] + layer * wbytes);
  bf16* dYt = reinterpret_cast<bf16*>(ws + W.dYt);
  bf16* Xt = reinterpret_cast<bf16*>(ws + W.Xt);
  float* dWd = reinterpret_cast<float*>(ws + W.dWd);
  const int ldk = W.ldk;
  if (want_dc)
    TRY(cara_colsum_bf16(dY, L.out, Mr, L.out, reinterpret_cast<float*>(ws + W.dc[L.slot]) + (size_t)layer * L.out, ws + W.xscratch, st));
  // dW = dY^T X as split-K slabs.  Straight from the row-major activations through the transposing-read GEMM when the shapes
  // allow (CARA_EXACT_TN=0: the first form -- two activation-sized transposes with zeroed pad columns, then one batched
  // launch of the default GEMM over the transposed copies)
  const size_t slab_stride = (size_t)L.out * L.in;
  int used = dw_slabs(L.out, L.in, Mr);
  static const int use_tn = env_once("CARA_EXACT_TN", 1);
  if (!(use_tn && cara_gemm_tn_f32(dY, L.out, X, L.in, dWd, L.in, L.out, L.in, Mr, used, slab_stride, st) == CARA_OK)) {
    used = W.nslab;
    if (ldk > Mr) {   // K of the dW product is Mr rounded up to 64: the pad columns of both transposes must be zero
      if (hipMemset2DAsync(dYt + Mr, (size_t)ldk * 2, 0, (size_t)(ldk - Mr) * 2, L.out, hs) != hipSuccess) return CARA_E_LAUNCH;
      if (hipMemset2DAsync(Xt + Mr, (size_t)ldk * 2, 0, (size_t)(ldk - Mr) * 2, L.in, hs) != hipSuccess) return CARA_E_LAUNCH;
    }
    TRY(cara_transpose_bf16_ld(dY, L.out, dYt, ldk, Mr, L.out, st));
    TRY(cara_transpose_bf16_ld(X, L.in, Xt, ldk, Mr, L.in, st));
    // split-K in one batched launch: slab z covers K columns [z * ldk/nslab, ...) of both transposes
    cara_gemm_args d = {};
    d.A = dYt; d.lda = ldk; d.B = Xt; d.ldb = ldk; d.M = L.out; d.N = L.in; d.K = ldk / used;
    d.epi = CARA_EPI_F32; d.C = dWd; d.ldc = L.in;
    d.batch = used; d.strideA = d.K; d.strideB = d.K; d.strideC = (long long)slab_stride;
    TRY(cara_gemm_bf16(&d, st));
  }
  TRY(cara_dropout_grad_contract(dWd, used, slab_stride, L.U, L.Vs, Rp, L.out, L.in, s->wd_p, s->wd_seed, (unsigned)(4 * layer + L.slot),
                                 reinterpret_cast<float*>(ws + W.dU[L.slot]) + (size_t)layer * L.in * Rp,
                                 reinterpret_cast<float*>(ws + W.dVs[L.slot]) + (size_t)layer * L.out * Rp, ws + W.xscratch, st));
  if (want_dx) {
    a.A = dY; a.lda = L.out; a.B = L.Wt; a.B3 = wefft; a.ldb = L.out; a.A2 = nullptr; a.B2 = nullptr; a.Rp = 0;
    a.M = Mr; a.N = L.in; a.K = L.out; a.bias = nullptr;
    if (a.ldc == 0) a.ldc = L.in;
    with_scratch(a, cx);
    TRY(cara_gemm_bf16(&a, st));
  }
  return CARA_OK;
}

void make_lins(const cara_geom* g, const cara_vit_weights* w, const char* pack, const cara_pack_layout& pl, int l, Lin* out) {
  const size_t D = g->dim;
  const char* pk = pack + (size_t)l * pl.layer_stride;
  auto B = [](const void* p, size_t elems) { return static_cast<const bf16*>(p) + elems; };
  auto P = [&](size_t off) { return reinterpret_cast<const bf16*>(pk + off); };
  out[0] = Lin{B(w->qkv_w, l * 3 * D * D), B(w->qkv_wt, l * 3 * D * D), P(pl.Ut_qkv), P(pl.U_qkv), P(pl.Vs_qkv), P(pl.Vst_qkv),
               w->qkv_b + (size_t)l * 3 * D, (int)D, (int)(3 * D), 0};
  out[1] = Lin{B(w->proj_w, l * D * D), B(w->proj_wt, l * D * D), P(pl.Ut_proj), P(pl.U_proj), P(pl.Vs_proj), P(pl.Vst_proj),
               reinterpret_cast<const float*>(pk + pl.bias_proj), (int)D, (int)D, 1};
  out[2] = Lin{B(w->fc1_w, l * 4 * D * D), B(w->fc1_wt, l * 4 * D * D), P(pl.Ut_fc1), P(pl.U_fc1), P(pl.Vs_fc1), P(pl.Vst_fc1),
               reinterpret_cast<const float*>(pk + pl.bias_fc1), (int)D, (int)(4 * D), 2};
  out[3] = Lin{B(w->fc2_w, l * 4 * D * D), B(w->fc2_wt, l * 4 * D * D), P(pl.Ut_fc2), P(pl.U_fc2), P(pl.Vs_fc2), P(pl.Vst_fc2),
               reinterpret_cast<const float*>(pk + pl.bias_fc2), (int)(4 * D), (int)D, 3};
  // CARA_GEMM_PACKED=0: stage the weights from their row-major images (A/B measurements)
  static const bool use_packed = env_once("CARA_GEMM_PACKED", 1) != 0;
  if (use_packed) {
    const void* wp[4][2] = {{w->qkv_wp, w->qkv_wtp}, {w->proj_wp, w->proj_wtp}, {w->fc1_wp, w->fc1_wtp}, {w->fc2_wp, w->fc2_wtp}};
    for (int i = 0; i < 4; ++i) {
      const size_t elems = (size_t)l * out[i].in * out[i].out;
      if (wp[i][0]) out[i].Wp = B(wp[i][0], elems);
      if (wp[i][1]) out[i].Wtp = B(wp[i][1], elems);
    }
  }
}

bool g_inside_enabled(int slot) {   // CARA_GEMM_G_INSIDE: bit 0 qkv, bit 1 fc1 (default 3: both)
  static const int v = env_once("CARA_GEMM_G_INSIDE", 3);
  return (v & (slot == 0 ? 1 : 2)) != 0;
}

// ---- The block plan: everything the forward of a block, its backward and the workspace layout decide about it, decided in one place.
// The switches and predicates of this section are read and called here only (plan_block, placements); the two passes take the plan. ----

// CARA_CLS_SHORTCUT=0 turns the exact last-block shortcut off (A/B measurements only)
bool cls_shortcut_enabled() {
  static const int v = env_once("CARA_CLS_SHORTCUT", 1);
  return v != 0;
}

// CARA_CLS_ATTN=0: the last block runs the full attention kernels although only its cls query matters (A/B measurements only)
bool cls_attention_enabled() {
  static const int v = env_once("CARA_CLS_ATTN", 1);
  return v != 0;
}

// CARA_DV (default 0; bit 0: fc1, bit 1: qkv): dVs (+ dc) of fc1 / qkv out of their dX GEMM's own A tiles on the 160 x 256 x 64 tile;
// the workspace then holds one slab per 160-row tile and K step for them (placements)
int dv_env() {
  static const int v = env_once("CARA_DV", 0);
  return v;
}

// CARA_FUSE_XU=0 keeps the K = dim adapter contractions (T = LN(x) U of qkv / fc1, G' = dY Vs of proj / fc2) as
// separate cara_skinny_xu passes instead of fusing them into the LayerNorm kernels
bool fuse_xu(const cara_geom* g) {
  static const int v = env_once("CARA_FUSE_XU", 1);
  return v != 0 && (g->Rp == 32 || g->Rp == 64) && cara_layernorm_takes(g->dim, true);
}

// CARA_PANEL_ACTS = mask of the activation groups written K-panel-major ([K/32][M][32], cara_gemm_args::c_panels /
// a_panels) so that the GEMM that consumes them stages whole cache lines: 1 = h / dH (written by GEMM epilogues),
// 2 = xn1 / xn2 (LayerNorm forward), 4 = the dY of fc2 / proj (LayerNorm backward).  Default 5: group 2 costs
// 0.2 ms per step although the GEMMs reading xn1 / xn2 gain 5-8 us each when timed alone.
// Not in the exact-dropout mode, not on the cls-row-only last block.
bool panel_acts(int Mr, const cara_vit_shape* s, int what) {
  static const int v = env_once("CARA_PANEL_ACTS", 5);
  return (v & what) != 0 && !s->wd_exact && Mr >= 1024;
}

// CARA_SAVE_GELU_GRAD (default: on where CARA_EPI_RIDERS is): fc1 forward keeps gelu'(u) (IEEE half) instead of the pre-activation u, and
// the fc2 dX epilogue is one multiply per element instead of the erf arithmetic (CARA_EPI_GELU_DG / CARA_EPI_MULH, include/cara_hip.h).
// Where the LayerNorms compute T = X U (the forward's fc1 GEMM then never has the adapter inside, a form the new epilogue does not
// take), factored mode.  Measured alone (r04, same box): a tie -- fc1 forward 77.3 -> 80.0 us, fc2 dX 76.9 -> 74.3: neither epilogue is
// bound by its VALU count any more (docs/findings/r04.md section 6).
static int epi_riders_env() {
  static const int v = env_once("CARA_EPI_RIDERS", 0);
  return v;
}
bool save_gelu_grad(const cara_geom* g, const cara_vit_shape* s) {
  static const int v = env_once("CARA_SAVE_GELU_GRAD", -1);
  return (v < 0 ? epi_riders_env() != 0 : v != 0) && fuse_xu(g) && !s->wd_exact;
}

// CARA_EPI_RIDERS (default 0): fc1's dVs = dH^T T (+ dc) and fc2's dU = h^T G' are computed by the epilogue of the fc2 dX GEMM, on the dH
// tile it has just produced and the h tile at the same coordinates (cara_gemm_args::er_*), instead of as workgroups riding in the fc1 dX
// launch that re-read dH and h (154 MB per block at the headline shape); the fc1 dX launch then carries nothing and runs on the
// 160 x 256 x 64 tile.  Rank <= 16, full-size blocks; what the shape allows is asked of cara_gemm_epi_rider_chunks() at the launch.
// Measured (r04, same box, profiles/r04_n_*): fc1 dX 86.4 -> 56.2 us, fc2 dX 74.3 -> 102.8 us, and the end-of-pass slab sums read
// 99 slabs per product instead of 6 (+80 us per step): 8.005 -> 8.096 ms per step.  The riders' epilogue is a longer DEPENDENT chain
// per wave (two operand streams, an LDS round trip more per row tile) in a launch that is bound by such chains, not by any unit
// (MFMA-busy 0.25, LDS 24 %, +105 MB of reads at 3.5 TB/s): off.
bool epi_riders_geom(const cara_geom* g, int Mr, bool exact) {
  const int v = epi_riders_env();
  cara_vit_shape sh = {};
  sh.wd_exact = exact ? 1 : 0;
  return v != 0 && !exact && save_gelu_grad(g, &sh) && g->Rp == 32 && g->rank > 0 && g->rank <= 16 && Mr > 1024 && (Mr & 3) == 0 && 4 * g->dim >= 3072 && ((4 * g->dim) & 127) == 0;
}

Placements placements(const cara_geom* g, const cara_vit_shape* s, int rows) {
  return Placements{epi_riders_geom(g, rows, s->wd_exact != 0), dv_env() != 0 && g->Rp == 32};
}

// Does the 160 x 256 x 64 tile really take this product of the model?  cara_gemm8_policy looks at the shape only; the tile's
// adapter-inside path and its riders are built for one r-tile (cara_gemm8_plan: Rp = 32, rank <= 16).  The activation LAYOUT
// (K-panel-major h / dH for the 128-tile family, row-major for the tile) must follow what will run: at rank 64 the shape-only
// answer left fc2 forward on the 128-tile kernel reading row-major A (9.696 -> 9.75 ms on the rank-64 leg).
bool tile_policy(const cara_geom* g, int M, int N, int K, int riders) {
  return g->Rp == 32 && g->rank > 0 && g->rank <= 16 && cara_gemm8_policy(M, N, K, riders);
}

struct BlockPlan {
  // Rows.  Only the cls token of the LAST block's output reaches the logits (timm takes x[:, 0] after the final norm), and proj /
  // LayerNorm-2 / fc1 / fc2 act per token: in the last block they run on the B cls rows only (row stride N * D).  Exact, not an
  // approximation: every other row of that block's proj / MLP output is dead, and only the cls rows carry gradient into them.  qkv and
  // attention still see all tokens (keys / values); with cls_attn only the cls query runs (only that row of the output is read).
  bool cls_only, cls_attn;
  int Mr, ldr, rps;   // rows of the proj / MLP half (M or B), row stride of the residual-stream rows used, rows per sample for DropPath
  // Mode: exact weight dropout (plain GEMMs on the merged weights); order 2 (the QKV linear in the dense-delta form); no backward will
  // follow (cara_vit_shape::inference: the forward does not keep what only it reads); fx: the LayerNorm kernels compute the K = dim
  // adapter contractions (T of qkv / fc1, G' of fc2), fxp: and LayerNorm-2 backward the G' of proj (CARA_LN2B_XU=0: proj's dX GEMM does,
  // except on the cls rows); fc1 forward keeps gelu'(u) instead of u (CARA_EPI_GELU_DG / CARA_EPI_MULH)
  bool exact, dense_qkv, inference, fx, fxp, save_gelu_grad;
  // Layout of each 16-bit activation the block writes or reads: rows per K-panel, 0 = row-major (Act).  xn1 and the dyb left for the
  // block below have all M rows, the others Mr.  (Order 2: xn1 stays row-major -- the dense dD = xn1^T dY of the backward reads it with
  // transposing LDS reads.  h is row-major where fc2 forward runs on the 160 x 256 x 64 tile, which stages whole 128-byte lines of
  // row-major operands, dH where fc1 dX does.  The last block's dyb comes from the final norm's backward: row-major, on the cls rows.)
  int xn1, xn2, h, dH, dyp, dyb_in, dyb_out;
  // Gradient enters the token stream only through the cls rows.  With the last block on its cls rows every kernel of that block reads
  // dx / dyb on those rows only, and its LayerNorm-1 backward -- the first launch that touches every row of dx -- is told so (dx_in on
  // every N-th row): the two buffers need no zeroing (58 MB of memset + 39 MB of zeros read back, ~18 us per step, r05).  Otherwise
  // (CARA_CLS_SHORTCUT=0, exact weight dropout, CARA_BWD_MEMSETS=1 for A/B runs) the pass starts with the memsets and reads every row.
  bool dx_on_cls;
  int dx_in_every;
  // Which launch of the backward computes which products (proj: always Own).  The placements other than Own are measured and off
  // (DESIGN.md 7.3); all need launches that carry products (fuse_ts), one r-tile and the factored mode, and exclude one another.
  Riders fc2 = Riders::Own, fc1 = Riders::Own, qkv = Riders::Own;
};
BlockPlan plan_block(const cara_geom* g, const cara_vit_shape* s, int M, int l) {
  static const int fc1_side = env_once("CARA_FC1_SIDE", 0);
  static const int ln2b_xu = env_once("CARA_LN2B_XU", 1);
  static const int force_zero = env_once("CARA_BWD_MEMSETS", 0);
  const int D = g->dim, N = s->tokens;
  const bool last = l == g->depth - 1;
  BlockPlan p;
  p.exact = s->wd_exact != 0;
  p.dense_qkv = g->cp_length == 2;
  p.inference = s->inference != 0 && !p.exact;
  p.cls_only = last && cls_shortcut_enabled() && !p.exact && s->pool == 0;   // (a pooled readout reads every patch row of the last block)
  p.cls_attn = p.cls_only && cls_attention_enabled();
  const int Mr = p.Mr = p.cls_only ? s->B : M;
  p.ldr = p.cls_only ? N * D : D;
  p.rps = p.cls_only ? 1 : N;
  p.fx = fuse_xu(g) && !p.exact;
  p.fxp = p.fx && (ln2b_xu != 0 || p.cls_only);
  p.save_gelu_grad = save_gelu_grad(g, s);
  p.dx_on_cls = p.cls_only && !force_zero;
  p.dx_in_every = p.dx_on_cls ? N : 0;
  p.xn1 = panel_acts(M, s, 2) && !p.dense_qkv ? M : 0;
  p.xn2 = panel_acts(Mr, s, 2) ? Mr : 0;
  p.h = panel_acts(Mr, s, 1) && !tile_policy(g, Mr, D, 4 * D, 0) ? Mr : 0;
  p.dyp = panel_acts(Mr, s, 4) ? Mr : 0;
  p.dyb_out = panel_acts(M, s, 4) ? M : 0;
  p.dyb_in = last ? 0 : p.dyb_out;
  const bool one_rtile = g->Rp == 32 && g->rank > 0 && g->rank <= 16;
  const bool can = !p.exact && one_rtile && fuse_ts(Mr, g->Rp);
  const Placements open = placements(g, s, Mr);
  const bool fc1_tile = g_inside_enabled(2) && tile_policy(g, Mr, D, 4 * D, 0);   // fc1's dX GEMM without riders runs on the 160 x 256 x 64 tile
  if (can && !open.a_tiles && open.epilogue) {
    p.fc2 = Riders::Epilogue;
    p.fc1 = Riders::DoneAbove;
  } else if (can && !p.cls_only && (dv_env() & 1) && fc1_tile) {
    p.fc2 = Riders::BothHome;
    p.fc1 = Riders::ATiles;
  } else if (can && fc1_side != 0 && fc1_tile && side_stream() != nullptr) {
    p.fc1 = Riders::Side;
  }
  if (can && !p.cls_only && (dv_env() & 2) && g_inside_enabled(0) && tile_policy(g, M, D, 3 * D, 0)) p.qkv = Riders::ATiles;
  p.dH = panel_acts(Mr, s, 1) && !tile_policy(g, Mr, D, 4 * D, p.fc1 == Riders::Own ? 1 : 0) ? Mr : 0;
  return p;
}

// tiny classifier-head backward (B x classes x D, fp32 VALU).  The three outputs are independent: blocks
// [0, nbw) take dW (and db), the rest dxn, so the two long loops run side by side instead of one after the other in
// every thread (58 -> ~25 us; it sits alone at the head of the backward pass)
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ dl, const bf16* __restrict__ xn,
                                                       const float* __restrict__ W, float* __restrict__ dW,
                                                       float* __restrict__ db, bf16* __restrict__ dxn, int B, int Cn, int D, int nbw,
                                                       const float* __restrict__ loss_scale, float* __restrict__ found_inf) {
  if ((int)blockIdx.x < nbw) {
    // the two gradients this kernel FINISHES leave unscaled (cara_vit_shape::loss_scale); dxn stays in the scaled domain
    const float gs = loss_scale ? 1.f / *loss_scale : 1.f;
    const int e = blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (e < Cn * D) {
      const int c = e / D, d = e - c * D;
      float s = 0.f;
#pragma unroll 8
      for (int b = 0; b < B; ++b) s += dl[b * Cn + c] * (float)xn[b * D + d];
      s *= gs;
      bad |= !(fabsf(s) <= 3.0e38f);
      dW[e] = s;
    }
    if (e < Cn) {
      float s = 0.f;
      for (int b = 0; b < B; ++b) s += dl[b * Cn + e];
      s *= gs;
      bad |= !(fabsf(s) <= 3.0e38f);
      db[e] = s;
    }
    if (found_inf && bad) *found_inf = 1.f;
  } else {
    const int e = (blockIdx.x - nbw) * 256 + threadIdx.x;
    if (e < B * D) {
      const int b = e / D, d = e - b * D;
      float s = 0.f;
#pragma unroll 10
      for (int c = 0; c < Cn; ++c) s += dl[b * Cn + c] * W[c * D + d];
      dxn[e] = (bf16)s;
    }
  }
}

// Final LayerNorm of one cls row + the classifier head in fp32 (cara_head_forward): workgroup (class chunk of HEAD_CHUNK, sample).
// Every workgroup normalises its sample's row itself (D floats: cheaper than a launch boundary); chunk 0 also writes the
// 16-bit xn row and mean / rstd for the backward.  The dot products run one class per wave and step over the row in float4
// pieces (a wave instruction reads 1 KiB of a head_w row), two classes in flight per wave.  A chunk is 16 classes = two rounds of
// the four waves: with 128 (64 workgroups for 64 x 100 logits, 13 dependent rounds each) the launch took 29 us (profiles/r05_g_*).
constexpr int HEAD_CHUNK = 16;
__global__ __launch_bounds__(256) void head_fwd_f32_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ Wh,
                                                           const float* __restrict__ bh, bf16* __restrict__ xn16,
                                                           float* __restrict__ mean, float* __restrict__ rstd,
                                                           float* __restrict__ logits, int Cn, int D, float eps) {
  __shared__ __attribute__((aligned(16))) float xs[1024];
  __shared__ float red[8];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* xr = x + (size_t)b * ldx;
  float s = 0.f;
  for (int d = tid; d < D; d += 256) { const float v = xr[d]; xs[d] = v; s += v; }
  s = wave_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  const float mu = ((red[0] + red[1]) + (red[2] + red[3])) / (float)D;
  float q = 0.f;
  for (int d = tid; d < D; d += 256) { const float a = xs[d] - mu; q += a * a; }
  q = wave_sum(q);
  if (lane == 0) red[4 + wave] = q;
  __syncthreads();
  const float rs = rsqrtf(((red[4] + red[5]) + (red[6] + red[7])) / (float)D + eps);
  for (int d = tid; d < D; d += 256) {
    const float v = (xs[d] - mu) * rs * gamma[d] + beta[d];
    xs[d] = v;
    if (blockIdx.x == 0) xn16[(size_t)b * D + d] = (bf16)v;
  }
  if (blockIdx.x == 0 && tid == 0) { mean[b] = mu; rstd[b] = rs; }
  __syncthreads();
  const int c0 = blockIdx.x * HEAD_CHUNK, c1 = c0 + HEAD_CHUNK < Cn ? c0 + HEAD_CHUNK : Cn;
  const int nd4 = D >> 2;   // float4 pieces of a row (D % 4 == 0)
  for (int c = c0 + wave * 2; c < c1; c += 8) {
    const int ca = c, cb = c + 1 < c1 ? c + 1 : c;
    const float4* wa = reinterpret_cast<const float4*>(Wh + (size_t)ca * D);
    const float4* wb = reinterpret_cast<const float4*>(Wh + (size_t)cb * D);
    float da = 0.f, db = 0.f;
    for (int i = lane; i < nd4; i += 64) {
      const float4 xv = *reinterpret_cast<const float4*>(xs + 4 * i);
      const float4 a = wa[i], bq = wb[i];
      da += (a.x * xv.x + a.y * xv.y) + (a.z * xv.z + a.w * xv.w);
      db += (bq.x * xv.x + bq.y * xv.y) + (bq.z * xv.z + bq.w * xv.w);
    }
    da = wave_sum(da);
    db = wave_sum(db);
    if (lane == 0) {
      logits[(size_t)b * Cn + ca] = da + bh[ca];
      if (cb != ca) logits[(size_t)b * Cn + cb] = db + bh[cb];
    }
  }
}

}  // namespace

extern "C" int cara_head_forward(const float* x, long ldx, const float* gamma, const float* beta, const float* head_w,
                                 const float* head_b, void* xn_16, float* mean, float* rstd, float* logits, int B, int classes,
                                 int D, float eps, void* stream) {
  if (!x || !gamma || !beta || !head_w || !head_b || !xn_16 || !mean || !rstd || !logits || B <= 0 || classes <= 0 || D <= 0 ||
      D > 1024 || (D & 3) || ldx < D)
    return CARA_E_ARG;
  hipLaunchKernelGGL(head_fwd_f32_kernel, dim3((classes + HEAD_CHUNK - 1) / HEAD_CHUNK, B), dim3(256), 0, static_cast<hipStream_t>(stream),
                     x, ldx, gamma, beta, head_w, head_b, (bf16*)xn_16, mean, rstd, logits, classes, D, eps);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}

extern "C" int cara_profile_sites(unsigned long long mask, int every) {
  if (mask && !g_prof.made) {
    for (int i = 0; i < CARA_SITE_COUNT; ++i)
      for (int k = 0; k < CARA_SITE_RING; ++k)
        for (int j = 0; j < 3; ++j)
          if (hipEventCreate(&g_prof.ev[i][k][j]) != hipSuccess) return CARA_E_LAUNCH;
    g_prof.made = true;
  }
  g_prof.mask = mask & ((1ull << CARA_SITE_COUNT) - 1);
  g_prof.every = every > 0 ? every : 1;
  for (int i = 0; i < CARA_SITE_COUNT; ++i) g_prof.n[i] = 0;
  return CARA_OK;
}

// avg_ms = mean (event 0 -> event 1) around the site's kernel(s) MINUS marker_ms = mean (event 1 -> event 2) with
// nothing between: two event records in a row are ~6-8 us apart on this stack, and that gap is inside every bracket
extern "C" int cara_profile_site_read(int site, float* avg_ms, float* marker_ms, int* launches) {
  if (site < 0 || site >= CARA_SITE_COUNT || !avg_ms || !marker_ms || !launches || !g_prof.made) return CARA_E_ARG;
  const long n = g_prof.n[site];
  *launches = 0;
  if (n == 0) return CARA_OK;
  double tot = 0, gap = 0;
  const int cnt = n < CARA_SITE_RING ? (int)n : CARA_SITE_RING;
  for (int i = 0; i < cnt; ++i) {
    float ms = 0.f, g = 0.f;
    if (hipEventElapsedTime(&ms, g_prof.ev[site][i][0], g_prof.ev[site][i][1]) != hipSuccess) return CARA_E_LAUNCH;
    if (hipEventElapsedTime(&g, g_prof.ev[site][i][1], g_prof.ev[site][i][2]) != hipSuccess) return CARA_E_LAUNCH;
    tot += ms;
    gap += g;
  }
  *marker_ms = (float)(gap / cnt);
  *avg_ms = (float)((tot - gap) / cnt);
  *launches = (int)n;   // brackets recorded since cara_profile_sites(); the averages cover the last min(n, CARA_SITE_RING)
  return CARA_OK;
}

extern "C" size_t cara_vit_workspace_bytes(const cara_geom* g, const cara_vit_shape* s) {
  Ws w;
  return layout(g, s, &w) ? w.total : 0;
}

static int head_backward_scaled(const float* dlogits, const void* xn, const float* head_w, float* dhead_w, float* dhead_b, void* dxn,
                                int B, int classes, int D, const float* loss_scale, float* found_inf, void* stream) {
  if (!dlogits || !xn || !head_w || !dhead_w || !dhead_b || !dxn || B <= 0 || classes <= 0 || D <= 0) return CARA_E_ARG;
  const int nbw = (classes * D + 255) / 256, nbx = (B * D + 255) / 256;
  hipLaunchKernelGGL(head_bwd_kernel, dim3(nbw + nbx), dim3(256), 0, static_cast<hipStream_t>(stream), dlogits,
                     (const bf16*)xn, head_w, dhead_w, dhead_b, (bf16*)dxn, B, classes, D, nbw, loss_scale, found_inf);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}
extern "C" int cara_head_backward(const float* dlogits, const void* xn, const float* head_w, float* dhead_w,
                                  float* dhead_b, void* dxn, int B, int classes, int D, void* stream) {
  return head_backward_scaled(dlogits, xn, head_w, dhead_w, dhead_b, dxn, B, classes, D, nullptr, nullptr, stream);
}

// The image of a forward is a cara_feed (common.h; the patch rows are feed.hip's): an fp32 batch, or resident uint8 pixels with
// their per-channel mean / std -- the batch itself, or a whole split of n_split images that `rows` indexes, each sample read whole or
// through its box, RandAugmented, mixed with a partner, colour-jittered / erased, all of its patches or a kept subset.  Each entry checks and sets
// the fields it has arguments for; the body adds the shape's, and everything behind the patch rows is the same.
// (a source of Hs x Ws images; an entry without a size of its own reads the shape's img x img images.  Fields are set by name: a
// field added to cara_feed must not shift an initialiser.)
static int img_of(const cara_vit_shape* s) { return s ? s->img : 0; }
static cara_feed source_of(int Hs, int Ws) {
  cara_feed f = {};
  f.Hs = Hs; f.Ws = Ws;
  return f;
}

// the activations a block's forward saves for its backward, each in the layout the plan gives it
struct Saved { Act xn1, ao, xn2, h; };
static Saved saved_acts(const Ctx& cx, const LayerWs& lw, int D, const BlockPlan& p) {
  return Saved{cx.act(lw.xn1, D, p.xn1), cx.act(lw.ao, p.ldr), cx.act(lw.xn2, D, p.xn2), cx.act(lw.h, 4 * D, p.h)};
}

static int vit_forward_body(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w, const cara_cp* cp, const float* head_w,
                            const float* head_b, const cara_feed& src, const float* droppath, void* workspace, float* logits, void* stream) {
  Ws W;
  if (!layout(g, s, &W) || !w || !cp || !head_w || !head_b || !workspace || !logits) return CARA_E_ARG;
  // an entry without a keep table writes the grid's patch rows, all of them: fewer tokens than that is the keep entries' alone
  const int grid = (s->img / s->patch) * (s->img / s->patch);
  if (!src.keep && s->tokens != grid + 1) return CARA_E_ARG;
  char* ws = static_cast<char*>(workspace);
  const int D = g->dim, M = W.M, Rp = g->Rp, B = s->B, N = s->tokens, P = N - 1;
  const float att_scale = 1.0f / sqrtf((float)(D / g->heads));
  cara_pack_layout pl;
  TRY(cara_pack_offsets(g, &pl));
  TRY(cara_factor_prep(g, cp, w->proj_b, w->fc1_b, w->fc2_b, ws + W.pack, stream));
  if (g->cp_length == 2) TRY(cara_dense_delta_materialize(g, cp, ws + W.dd, ws + W.ddt, stream));   // (order 2: BlockPlan::dense_qkv)
  // patch embedding: Conv2d(k = s = patch) as a GEMM over im2col rows, then cls + pos_embed
  const int kp = s->chans * s->patch * s->patch;
  cara_feed feed = src;
  feed.K = src.keep ? P : 0;
  feed.B = B; feed.C = s->chans; feed.Hi = feed.Wi = s->img; feed.p = s->patch;
  TRY(cara_feed_patch_rows(feed, ws + W.patches, stream));
  cara_gemm_args a = {};
  a.A = ws + W.patches; a.lda = kp; a.B = w->patch_w; a.ldb = kp; a.M = B * P; a.N = D; a.K = kp;
  a.bias = w->patch_b; a.epi = CARA_EPI_F32; a.C = ws + W.emb; a.ldc = D;
  const Ctx px{stream, ws, &W, s, Rp, W.ldt, g->rank};
  with_scratch(a, px);
  TRY(cara_gemm_bf16(&a, stream));
  if (src.keep) TRY(cara_assemble_tokens_keep(px.f32(W.emb), w->cls, w->pos, src.keep, px.f32(W.layer[0].x_in), B, P, grid, D, stream));
  else TRY(cara_assemble_tokens(px.f32(W.emb), w->cls, w->pos, px.f32(W.layer[0].x_in), B, P, D, stream));
  for (int l = 0; l < g->depth; ++l) {
    const BlockPlan p = plan_block(g, s, M, l);
    const LayerWs& lw = W.layer[l];
    Lin lin[4];
    make_lins(g, w, ws + W.pack, pl, l, lin);
    float *x_in = px.f32(lw.x_in), *x_mid = px.f32(lw.x_mid), *x_out = px.f32(l + 1 < g->depth ? W.layer[l + 1].x_in : W.x_last);
    const float *dp1 = droppath ? droppath + (size_t)(2 * l) * B : nullptr, *dp2 = droppath ? droppath + (size_t)(2 * l + 1) * B : nullptr;
    const Ctx cx = px.on(lw, l, p.Mr, !p.cls_only), cx_all = px.on(lw, l, M, true);   // (qkv and attention always run on all token rows)
    const Saved sv = saved_acts(cx, lw, D, p);
    auto linear = [&](int i, const Act& X, const cara_gemm_args& e, const Ctx& c, bool have_T = false) {
      return p.exact ? lin_fwd_exact(lin[i], X, e, c) : lin_fwd(lin[i], X, e, c, have_T);
    };
    // x = x + drop_path(attn(norm1(x)))
    {
      SiteBracket sb(CARA_SITE_LN1_FWD, cx_all);
      TRY(cara_layernorm_fwd_ex(x_in, D, w->ln1_g + (size_t)l * D, w->ln1_b + (size_t)l * D, sv.xn1.p, px.f32(lw.mean1), px.f32(lw.rstd1), M, D, s->eps,
                                (p.fx && !p.dense_qkv) ? lin[0].Ut : nullptr, g->rank, Rp, ws + lw.T[0], ws + lw.Tt[0], W.ldt, sv.xn1.panels, stream));
    }
    cara_gemm_args e = {};
    e.epi = CARA_EPI_BF16; e.C = ws + lw.qkv;
    if (p.dense_qkv) TRY(lin_fwd_dense(lin[0], sv.xn1, e, cx_all));
    else TRY(linear(0, sv.xn1, e, cx_all, p.fx));
    {
      SiteBracket sb(CARA_SITE_ATTN_FWD, cx_all);
      TRY((p.cls_attn ? cara_attention_cls_fwd : cara_attention_fwd)(ws + lw.qkv, ws + lw.ao, px.f32(lw.lse), B, N, g->heads, att_scale, stream));
    }
    e = {};
    e.epi = CARA_EPI_RESID; e.C = x_mid; e.aux = x_in; e.rowscale = dp1; e.rows_per_sample = p.rps; e.ldc = p.ldr;
#ifdef CARA_ABLATE_RESID   // timing experiment only: the residual products with a plain bf16 epilogue (wrong results)
    e = {}; e.epi = CARA_EPI_BF16; e.C = ws + lw.u;
#endif
    TRY(linear(1, sv.ao, e, cx));
    // x = x + drop_path(mlp(norm2(x)))
    {
      SiteBracket sb(CARA_SITE_LN2_FWD, cx);
      TRY(cara_layernorm_fwd_ex(x_mid, p.ldr, w->ln2_g + (size_t)l * D, w->ln2_b + (size_t)l * D, sv.xn2.p, px.f32(lw.mean2), px.f32(lw.rstd2), p.Mr, D, s->eps,
                                p.fx ? lin[2].Ut : nullptr, g->rank, Rp, ws + lw.T[2], ws + lw.Tt[2], W.ldt, sv.xn2.panels, stream));
    }
    e = {};
    // what the backward's fc2 dX epilogue needs: gelu'(u) itself, kept as IEEE half (CARA_EPI_GELU_DG / _MULH), or the pre-activation u
    e.epi = p.save_gelu_grad ? CARA_EPI_GELU_DG : CARA_EPI_GELU;
    writes(e, sv.h);
    e.C2 = p.inference ? nullptr : ws + lw.u;   // (only read by the backward)
    TRY(linear(2, sv.xn2, e, cx, p.fx));
    e = {};
    e.epi = CARA_EPI_RESID; e.C = x_out; e.aux = x_mid; e.rowscale = dp2; e.rows_per_sample = p.rps; e.ldc = p.ldr;
#ifdef CARA_ABLATE_RESID
    e = {}; e.epi = CARA_EPI_BF16; e.C = ws + lw.u;
#endif
    TRY(linear(3, sv.h, e, cx));
  }
  if (W.pool) {
    // pooled readout: mean of the patch rows (no LayerNorm in front) -> fc_norm (norm_g / norm_b carry it) -> head, the same fp32 launch
    TRY(cara_token_mean(px.f32(W.x_last), B, N, 1, D, px.f32(W.pooled), stream));
    return cara_head_forward(px.f32(W.pooled), (long)D, w->norm_g, w->norm_b, head_w, head_b, ws + W.clsn, px.f32(W.meanF), px.f32(W.rstdF), logits, B,
                             s->num_classes, D, s->eps, stream);
  }
  // norm -> cls token -> head  (LayerNorm is per token, so only the cls rows are normalised)
  // ... all in fp32, one launch (cara_head_forward): the 16-bit xn and the row statistics are kept for the backward
  return cara_head_forward(px.f32(W.x_last), (long)N * D, w->norm_g, w->norm_b, head_w, head_b, ws + W.clsn, px.f32(W.meanF), px.f32(W.rstdF), logits, B,
                           s->num_classes, D, s->eps, stream);
}

extern "C" int cara_vit_forward(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w,
                                const cara_cp* cp, const float* head_w, const float* head_b, const float* images,
                                const float* droppath, void* workspace, float* logits, void* stream) {
  if (!images) return CARA_E_ARG;
  cara_feed src = source_of(img_of(s), img_of(s));
  src.images = images;
  return vit_forward_body(g, s, w, cp, head_w, head_b, src, droppath, workspace, logits, stream);
}

extern "C" int cara_vit_forward_u8(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w,
                                   const cara_cp* cp, const float* head_w, const float* head_b, const unsigned char* pixels,
                                   const float* mean, const float* stdv, const float* droppath, void* workspace, float* logits,
                                   void* stream) {
  if (!pixels || !mean || !stdv) return CARA_E_ARG;
  cara_feed src = source_of(img_of(s), img_of(s));
  src.pixels = pixels; src.mean = mean; src.stdv = stdv;
  return vit_forward_body(g, s, w, cp, head_w, head_b, src, droppath, workspace, logits, stream);
}

extern "C" int cara_vit_forward_u8_rows(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w,
                                        const cara_cp* cp, const float* head_w, const float* head_b, const unsigned char* pixels,
                                        int n_split, const int64_t* rows, const float* mean, const float* stdv,
                                        const float* droppath, void* workspace, float* logits, int* bad, void* stream) {
  if (!pixels || !rows || n_split <= 0 || !mean || !stdv) return CARA_E_ARG;
  cara_feed src = source_of(img_of(s), img_of(s));
  src.pixels = pixels; src.mean = mean; src.stdv = stdv; src.n_split = n_split; src.rows = rows; src.bad = bad;
  return vit_forward_body(g, s, w, cp, head_w, head_b, src, droppath, workspace, logits, stream);
}

extern "C" int cara_vit_forward_u8_rows_crop(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w,
                                             const cara_cp* cp, const float* head_w, const float* head_b, const unsigned char* pixels,
                                             int n_split, int Hs, int Ws, const int64_t* rows, const int* boxes, const float* mean,
                                             const float* stdv, const float* droppath, void* workspace, float* logits, int* bad,
                                             void* stream) {
  if (!pixels || !rows || !boxes || n_split <= 0 || Hs <= 0 || Ws <= 0 || !mean || !stdv) return CARA_E_ARG;
  cara_feed src = source_of(Hs, Ws);
  src.pixels = pixels; src.mean = mean; src.stdv = stdv; src.n_split = n_split; src.rows = rows; src.bad = bad;
  src.boxes = boxes;
  return vit_forward_body(g, s, w, cp, head_w, head_b, src, droppath, workspace, logits, stream);
}

extern "C" int cara_vit_forward_u8_rows_mix(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w,
                                            const cara_cp* cp, const float* head_w, const float* head_b, const unsigned char* pixels,
                                            int n_split, int Hs, int Ws, const int64_t* rows, const int* boxes, const int* mix,
                                            const float* mean, const float* stdv, const float* droppath, void* workspace, float* logits,
                                            int* bad, void* stream) {
  if (!pixels || !rows || !mix || n_split <= 0 || Hs <= 0 || Ws <= 0 || !mean || !stdv) return CARA_E_ARG;
  cara_feed src = source_of(Hs, Ws);
  src.pixels = pixels; src.mean = mean; src.stdv = stdv; src.n_split = n_split; src.rows = rows; src.bad = bad;
  src.boxes = boxes; src.mix = mix;
  return vit_forward_body(g, s, w, cp, head_w, head_b, src, droppath, workspace, logits, stream);
}

extern "C" int cara_vit_forward_u8_rows_aug(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w,
                                            const cara_cp* cp, const float* head_w, const float* head_b, const unsigned char* pixels,
                                            int n_split, int Hs, int Ws, const int64_t* rows, const int* boxes, const int* mix,
                                            const int* aug, void* stat_scratch, const float* mean, const float* stdv,
                                            const float* droppath, void* workspace, float* logits, int* bad, void* stream) {
  if (!pixels || !rows || !aug || !stat_scratch || n_split <= 0 || Hs <= 0 || Ws <= 0 || !mean || !stdv) return CARA_E_ARG;
  cara_feed src = source_of(Hs, Ws);
  src.pixels = pixels; src.mean = mean; src.stdv = stdv; src.n_split = n_split; src.rows = rows; src.bad = bad;
  src.boxes = boxes; src.mix = mix; src.aug = aug; src.stat = stat_scratch;
  return vit_forward_body(g, s, w, cp, head_w, head_b, src, droppath, workspace, logits, stream);
}

extern "C" int cara_vit_forward_keep(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w, const cara_cp* cp,
                                     const float* head_w, const float* head_b, const float* images, const int* keep,
                                     const float* droppath, void* workspace, float* logits, int* bad, void* stream) {
  if (!images || !keep) return CARA_E_ARG;
  cara_feed src = source_of(img_of(s), img_of(s));
  src.images = images; src.bad = bad; src.keep = keep;
  return vit_forward_body(g, s, w, cp, head_w, head_b, src, droppath, workspace, logits, stream);
}

extern "C" int cara_vit_forward_u8_rows_keep(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w, const cara_cp* cp,
                                             const float* head_w, const float* head_b, const unsigned char* pixels, int n_split, int Hs,
                                             int Ws, const int64_t* rows, const int* boxes, const int* mix, const int* aug,
                                             void* stat_scratch, const int* keep, const float* mean, const float* stdv,
                                             const float* droppath, void* workspace, float* logits, int* bad, void* stream) {
  if (!pixels || !rows || !keep || (aug && !stat_scratch) || n_split <= 0 || Hs <= 0 || Ws <= 0 || !mean || !stdv) return CARA_E_ARG;
  cara_feed src = source_of(Hs, Ws);
  src.pixels = pixels; src.mean = mean; src.stdv = stdv; src.n_split = n_split; src.rows = rows; src.bad = bad;
  src.boxes = boxes; src.mix = mix; src.aug = aug; src.stat = stat_scratch; src.keep = keep;
  return vit_forward_body(g, s, w, cp, head_w, head_b, src, droppath, workspace, logits, stream);
}

extern "C" int cara_vit_forward_u8_rows_ra(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w, const cara_cp* cp,
                                           const float* head_w, const float* head_b, const unsigned char* pixels, int n_split, int Hs,
                                           int Ws, const int64_t* rows, const int* boxes, const int* mix, const int* aug,
                                           void* stat_scratch, const int* ra, void* ra_scratch, const int* keep, const float* mean,
                                           const float* stdv, const float* droppath, void* workspace, float* logits, int* bad,
                                           void* stream) {
  if (!pixels || !rows || !ra || !ra_scratch || (aug && !stat_scratch) || n_split <= 0 || Hs <= 0 || Ws <= 0 || !mean || !stdv) return CARA_E_ARG;
  cara_feed src = source_of(Hs, Ws);
  src.pixels = pixels; src.mean = mean; src.stdv = stdv; src.n_split = n_split; src.rows = rows; src.bad = bad;
  src.boxes = boxes; src.mix = mix; src.aug = aug; src.stat = stat_scratch; src.ra = ra; src.ra_stat = ra_scratch; src.keep = keep;
  return vit_forward_body(g, s, w, cp, head_w, head_b, src, droppath, workspace, logits, stream);
}

extern "C" int cara_vit_backward(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w,
                                 const cara_cp* cp, const float* head_w, const float* dlogits, const float* droppath,
                                 void* workspace, const cara_cp* grads, float* dhead_w, float* dhead_b, void* stream) {
  Ws W;
  // a shape that says "inference" describes a workspace without the backward's regions (and a forward that kept nothing)
  if (s && s->inference != 0 && !s->wd_exact) return CARA_E_ARG;
  if (!layout(g, s, &W) || !w || !cp || !head_w || !dlogits || !workspace || !grads || !dhead_w || !dhead_b) return CARA_E_ARG;
  char* ws = static_cast<char*>(workspace);
  BwdPass pass;
  const SlabFormats& formats = pass.formats;
  const Ctx px{stream, ws, &W, s, g->Rp, W.ldt, g->rank, &pass};
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const int D = g->dim, M = W.M, Rp = g->Rp, B = s->B, N = s->tokens;
  const float att_scale = 1.0f / sqrtf((float)(D / g->heads));
  cara_pack_layout pl;
  TRY(cara_pack_offsets(g, &pl));
  BlockPlan plans[64];
  for (int l = 0; l < g->depth; ++l) plans[l] = plan_block(g, s, M, l);
  const BlockPlan& last = plans[g->depth - 1];
  float* dx = px.f32(W.dx);
  const Ws::Bwd& R = W.bwd;
  TRY(head_backward_scaled(dlogits, ws + W.clsn, head_w, dhead_w, dhead_b, ws + W.dclsn, B, s->num_classes, D, s->loss_scale,
                           s->found_inf, stream));
  const float* dp_last = droppath ? droppath + (size_t)(2 * (g->depth - 1) + 1) * B : nullptr;
  if (W.pool) {
    // pooled readout: fc_norm's backward on the B pooled rows, then the pooled gradient spread over the patch rows -- every element of
    // dx and of the last block's dyb is written once (zeros on the cls rows), in the memsets' place
    TRY(cara_layernorm_bwd(ws + W.dclsn, px.f32(W.pooled), (long)D, w->norm_g, px.f32(W.meanF), px.f32(W.rstdF), nullptr, px.f32(W.dpooled), nullptr, nullptr, 1,
                           B, D, stream));
    TRY(cara_token_mean_bwd(px.f32(W.dpooled), dp_last, B, N, 1, D, dx, ws + R.dyb_fc2, last.dyb_in, stream));
  } else {
    if (!last.dx_on_cls) {   // (the last block reads every row of dx and of its dyb: zeros outside the cls rows)
      if (hipMemsetAsync(dx, 0, (size_t)M * D * 4, hs) != hipSuccess) return CARA_E_LAUNCH;
      if (hipMemsetAsync(ws + R.dyb_fc2, 0, (size_t)M * D * 2, hs) != hipSuccess) return CARA_E_LAUNCH;
    }
    TRY(cara_layernorm_bwd(ws + W.dclsn, px.f32(W.x_last), (long)N * D, w->norm_g, px.f32(W.meanF), px.f32(W.rstdF), nullptr, dx, ws + R.dyb_fc2, dp_last, 1, B,
                           D, stream));
  }
  bool have_G_fc2 = false;   // G' of this block's fc2 was left by the LayerNorm backward of the block above
  for (int l = g->depth - 1; l >= 0; --l) {
    const BlockPlan& p = plans[l];
    const LayerWs& lw = W.layer[l];
    Lin lin[4];
    make_lins(g, w, ws + W.pack, pl, l, lin);
    const float* dp1 = droppath ? droppath + (size_t)(2 * l) * B : nullptr;
    const float* dp_prev = (droppath && l > 0) ? droppath + (size_t)(2 * (l - 1) + 1) * B : nullptr;
    const Ctx cx = px.on(lw, l, p.Mr, !p.cls_only), cx_all = px.on(lw, l, M, true);   // (attention and qkv always run on all token rows)
    // what the forward saved; the dY of the four linears (dyb and G'[3] of fc2 were written by the block above / the final norm's backward)
    const Saved sv = saved_acts(cx, lw, D, p);
    const Act dyb = cx.act(R.dyb_fc2, p.ldr, p.dyb_in), dH = cx.act(R.dH, 4 * D, p.dH), dyp = cx.act(R.dyb_proj, p.ldr, p.dyp), dQKV = cx.act(R.dQKV, 3 * D);
    auto linear = [&](int i, const Act& dY, const Act& X, bool want_dx, const cara_gemm_args& e, bool want_dc, const Ctx& c, Riders where, bool have_G = false) {
      return p.exact ? lin_bwd_exact(lin[i], dY, X, want_dx, e, want_dc, c) : lin_bwd(lin[i], dY, X, want_dx, e, want_dc, c, where, have_G);
    };
    // ---- mlp branch: dY = drop_path scale * dx (already in dyb) ----
    cara_gemm_args e = {};
    e.epi = p.save_gelu_grad ? CARA_EPI_MULH : CARA_EPI_DGELU; e.aux = ws + lw.u;
    writes(e, dH);
    pass.epilogue_ran = false;
    TRY(linear(3, dyb, sv.h, true, e, true, cx, p.fc2, have_G_fc2));
    const Riders fc1 = (p.fc1 == Riders::DoneAbove && !pass.epilogue_ran) ? Riders::Own : p.fc1;   // (the epilogue said no: fc1 carries its own)
    have_G_fc2 = false;
    e = {};
    e.epi = CARA_EPI_BF16; e.C = ws + W.dXn;
    TRY(linear(2, dH, sv.xn2, true, e, true, cx, fc1));
    // dyp = dY of this block's proj: with fxp its G' = dY Vs comes out of the same kernel
    {
      SiteBracket sb(CARA_SITE_LN2_BWD, cx);
      TRY(cara_layernorm_bwd_ex(ws + W.dXn, px.f32(lw.x_mid), p.ldr, w->ln2_g + (size_t)l * D, px.f32(lw.mean2), px.f32(lw.rstd2), dx, dx, dyp.p, dp1,
                                p.rps, p.Mr, D, p.fxp ? lin[1].Vst : nullptr, g->rank, Rp, ws + R.G[1], ws + R.Gt[1], W.ldt, dyp.panels, stream));
    }
    // ---- attention branch ----
    e = {};
    e.epi = CARA_EPI_BF16; e.C = ws + W.dAO; e.ldc = p.ldr;
    // (with cls_attn only the cls rows of dAO are ever read)
    if (p.cls_only && !p.cls_attn && hipMemsetAsync(ws + W.dAO, 0, (size_t)M * D * 2, hs) != hipSuccess) return CARA_E_LAUNCH;
    TRY(linear(1, dyp, sv.ao, true, e, true, cx, Riders::Own, p.fxp));
    {
      SiteBracket sb(CARA_SITE_ATTN_BWD, cx_all);
      TRY((p.cls_attn ? cara_attention_cls_bwd : cara_attention_bwd)(ws + lw.qkv, ws + lw.ao, ws + W.dAO, px.f32(lw.lse), dQKV.p, B, N, g->heads, att_scale,
                                                                     stream));
    }
    e = {};
    e.epi = CARA_EPI_BF16; e.C = ws + W.dXn;
    // block 0 has nothing trainable upstream of it: its dX GEMM and LayerNorm backward are skipped
    if (p.dense_qkv) TRY(lin_bwd_dense(lin[0], dQKV, sv.xn1, l > 0, e, cx_all));
    else TRY(linear(0, dQKV, sv.xn1, l > 0, e, false, cx_all, p.qkv));
    // the side stream's products read dH and G' of fc2, which the kernels below overwrite: the caller's stream waits for them (they
    // were launched some 300 us ago)
    if (pass.side_join) {
      if (hipStreamWaitEvent(hs, side_stream()->join, 0) != hipSuccess) return CARA_E_LAUNCH;
      pass.side_join = false;
    }
    if (l > 0) {
      // dyb = dY of fc2 of the block BELOW (all M rows there: only the last block runs on cls rows); this block's
      // fc2 is through with the buffer (stream order)
      Lin below[4];
      make_lins(g, w, ws + W.pack, pl, l - 1, below);
      SiteBracket sb(CARA_SITE_LN1_BWD, cx_all);
      TRY(cara_layernorm_bwd_rows_in(ws + W.dXn, px.f32(lw.x_in), D, w->ln1_g + (size_t)l * D, px.f32(lw.mean1), px.f32(lw.rstd1), dx, dx, dyb.p, dp_prev, N, M,
                                     D, p.fx ? below[3].Vst : nullptr, g->rank, Rp, ws + R.G[3], ws + R.Gt[3], W.ldt, p.dyb_out, p.dx_in_every, stream));
      have_G_fc2 = p.fx;
    }
  }
  TRY(flush_waiting(px));   // (block 0's proj dU still waits where its qkv is not lin_bwd's: order 2)
  if (!last.exact) {   // (the exact mode wrote dU / dVs / dc of every layer directly)
    const int ins[4] = {D, D, D, 4 * D}, outs[4] = {3 * D, D, 4 * D, D};
    const int L = g->depth;
    cara_ts_reduce red[CARA_TS_REDUCE_MAX];   // all slab sums of the pass in ONE launch (8 + 6 of them, more where a linear's layers differ in slab format)
    int nred = 0;
    const int Rc = (Rp == 32 && ts_rank(px) <= 16) ? 16 : 0;   // (every product of the pass was told the same rank)
    auto push = [&](const cara_ts_reduce& e) -> int {
      if (nred == CARA_TS_REDUCE_MAX) {
        TRY(cara_tskinny_reduce_many(red, nred, stream));
        nred = 0;
      }
      red[nred++] = e;
      return CARA_OK;
    };
    for (int i = 0; i < 4; ++i) {
      if (i == 0 && last.dense_qkv) continue;   // order 2: the QKV linear wrote no skinny slabs (its gradient is dense, below)
      float *dU = px.f32(W.dU[i]), *dVs = px.f32(W.dVs[i]), *dc = i == 0 ? nullptr : px.f32(W.dc[i]);
      // qkv (i == 0) sees all tokens in every block; proj / fc1 / fc2 of the last block ran on B rows where it is on its cls rows,
      // so that block's slabs have their own chunking
      const int full = (i == 0 || !last.cls_only) ? L : L - 1;
      // runs of layers whose products left the same slab format (one per block / one per wave: SlabFormats)
      auto runs = [&](const unsigned short* f, size_t slabs, size_t stride, float* out, float* colsum, int K1) -> int {
        for (int l0 = 0, l1; l0 < full; l0 = l1) {
          for (l1 = l0 + 1; l1 < full && f[l1] == f[l0];) ++l1;
          TRY(push(cara_ts_reduce{ws + slabs + l0 * stride, stride, out + (size_t)l0 * K1 * Rp, colsum ? colsum + (size_t)l0 * K1 : nullptr, l1 - l0, M, K1, Rp, Rc, f[l0]}));
        }
        return CARA_OK;
      };
      TRY(runs(formats.U[i], W.slabU[i], W.strideU[i], dU, nullptr, ins[i]));
      TRY(runs(formats.V[i], W.slabV[i], W.strideV[i], dVs, dc, outs[i]));
      if (i != 0 && last.cls_only) {
        const size_t l = L - 1;
        TRY(push(cara_ts_reduce{ws + W.slabU[i] + l * W.strideU[i], 0, dU + l * ins[i] * Rp, nullptr, 1, B, ins[i], Rp, Rc, 0}));
        TRY(push(cara_ts_reduce{ws + W.slabV[i] + l * W.strideV[i], 0, dVs + l * outs[i] * Rp, dc + l * outs[i], 1, B, outs[i], Rp, Rc, 0}));
      }
    }
    TRY(cara_tskinny_reduce_many(red, nred, stream));
  }
  const cara_layer_grads lg{px.f32(W.dU[0]), px.f32(W.dVs[0]), px.f32(W.dU[1]), px.f32(W.dVs[1]), px.f32(W.dU[2]), px.f32(W.dVs[2]),   // dU, dVs of qkv, proj, fc1
                            px.f32(W.dU[3]), px.f32(W.dVs[3]), px.f32(W.dc[1]),  px.f32(W.dc[2]),  px.f32(W.dc[3])};                      // ... fc2; dc of proj, fc1, fc2
  TRY(cara_factor_grad_reduce_ex(g, cp, &lg, grads, ws + W.gscratch, s->loss_scale, s->found_inf, stream));
  if (last.dense_qkv)   // CP_A1 / CP_A2 / CP_R1 of the order-2 tensorisation, from the dense dD of every (layer, projection)
    TRY(cara_dense_delta_grad(g, cp, px.f32(W.dD), grads, ws + W.dd_scratch, stream));
  return CARA_OK;
}

