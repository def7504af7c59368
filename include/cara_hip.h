/* cara_hip.h -- C ABI of libcara_hip.so, the MI355X (gfx950) CaRA hot path.
 *
 * The reference (BonnBytes/CaRA) is pure Python on PyTorch and has no FFI of its own: the
 * functions below are what a maintainer's ctypes binding replaces inside the two patched
 * forwards of /root/reference/src/cara/cara.py (cp_attn :15-60, cp_mlp :63-95) and around the
 * train step of image_classification/vit_cp.py:45-50.  INTEGRATION.md shows that binding.
 *
 * Conventions: plain pointers and sizes only (device pointers unless a comment says host);
 * every entry point enqueues work on `stream` (a hipStream_t passed as void*) and returns an
 * int status: 0 = ok, >0 = CARA_E_* below.  Nothing allocates, frees or synchronises, and nothing
 * keeps state between calls (the one exception is the opt-in diagnostic of cara_profile_sites), so
 * every call is re-entrant and hipGraph-capturable; all work of a call goes to the caller's stream.
 * The caller makes the device of its pointers and stream current (hipSetDevice) before calling.
 * bf16 tensors are raw uint16 (round-to-nearest-even of fp32).  All matrices are row-major and dense
 * unless an ld* is given.
 */
#ifndef CARA_HIP_H
#define CARA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CARA_OK 0
#define CARA_E_ARG 1     /* bad shape / null pointer / unsupported size */
#define CARA_E_LAUNCH 2  /* hipGetLastError() != hipSuccess after a launch */

/* ---- library info ------------------------------------------------------------------------ */
int cara_abi_version(void);              /* bumped on any signature change */
const char* cara_build_arch(void);       /* "gfx950" */
/* The 16-bit operand type of this build: "bf16" (libcara_hip.so) or "fp16" (libcara_hip_f16.so: the same sources compiled with
 * IEEE-half operands at the same MFMA rate -- every "bf16" below then reads "fp16"; same ABI, struct for struct).           */
const char* cara_operand_type(void);

/* ---- GEMM with rank-R K-extension -------------------------------------------------------- */
/* C = A[M,K] * B[N,K]^T  (+ A2[M,Rp] * B2[N,Rp]^T)  then an epilogue.  bf16 in, fp32 accumulate.
 * This is the adapter linear of cara.py:25-42,50-58,75-82,87-93 in factored form:
 * A2 = T = X U (cara_skinny_xu), B2 = Vs = s * g (.) V (cara_factor_prep), so that
 * y = X W^T + b + s((X U) (.) g) V^T + s c  costs Rp/K extra MFMA work instead of a second GEMM.
 * Requirements: K % 64 == 0, Rp in {0, 32, 64}; M, N arbitrary (edges are clamped/masked); each
 * operand spans < 4 GiB (32-bit byte offsets), else CARA_E_ARG.                                  */
enum {
  CARA_EPI_BF16 = 0,   /* C bf16 [M,ldc]          = acc + bias                                  */
  CARA_EPI_F32 = 1,    /* C fp32 [M,ldc]          = acc + bias                                  */
  CARA_EPI_GELU = 2,   /* C2 bf16 = u = acc+bias ; C bf16 = gelu_erf(u)           (fc1 forward) */
  CARA_EPI_RESID = 3,  /* C fp32 = aux_f32 + rowscale[m / rows_per_sample] * (acc + bias)       */
  CARA_EPI_DGELU = 4,  /* C bf16 = acc * gelu_erf'(aux_bf16[m,n])                (fc2 backward) */
  /* The same pair with the DERIVATIVE saved instead of the pre-activation: the forward has e = exp(-u^2/2) and the erf polynomial in  */
  /* registers for gelu(u) anyway (4 more VALU per element give gelu'(u) of the UNROUNDED u), and the backward epilogue is one multiply */
  /* instead of ~15 VALU per element of erf arithmetic in a launch whose epilogue is VALU-bound.  gelu' lies in [-0.13, 1.13]: it is kept */
  /* as IEEE half (11 significand bits) in BOTH builds of the library -- bf16's 8 bits would cost more than rounding u did.              */
  CARA_EPI_GELU_DG = 5, /* C bf16 = gelu_erf(u), u = acc+bias ; C2 fp16 = gelu_erf'(u) (NULL: not kept)         (fc1 forward) */
  CARA_EPI_MULH = 6,    /* C bf16 = acc * aux_fp16[m,n]                                                          (fc2 backward) */
};
typedef struct {
  const void* A;  int lda;      /* bf16 [M,K]  */
  const void* B;  int ldb;      /* bf16 [N,K]  */
  const void* A2; const void* B2; int Rp;   /* bf16 [M,Rp], [N,Rp]; Rp = 0 => none */
  int M, N, K;
  const float* bias;            /* fp32 [N] or NULL */
  int epi;
  void* C;  int ldc;
  void* C2;                     /* CARA_EPI_GELU / _GELU_DG only (same ldc); NULL = the pre-activation / derivative is not kept */
  const void* aux;              /* CARA_EPI_RESID: fp32 [M,ldc]; CARA_EPI_DGELU: bf16 [M,ldc]; CARA_EPI_MULH: fp16 [M,ldc] */
  const float* rowscale;        /* CARA_EPI_RESID: fp32 [M / rows_per_sample] or NULL (=1) */
  int rows_per_sample;
  void* scratch;                /* optional: cara_gemm_scratch_bytes() of caller memory, used by ONE call  */
  size_t scratch_bytes;         /* at a time.  With it, few-row products (M <= 128, K >= 512) cut their K  */
                                /* loop into slabs that run as one batched launch (fp32 partials there).   */
  int batch;                    /* > 1: `batch` independent products in ONE launch; product z uses A, B,  */
  long long strideA, strideB, strideC;   /* C advanced by z * stride (elements); no A2/B2/aux/C2 then     */
  /* Whole adapter inside the GEMM (Rp in {32, 64}, B2 set, A2 NULL): every tile also accumulates its rows of */
  /* T = A Ut^T (Ut bf16 [Rp, K], rows >= rank zero: the operand cara_skinny_xu takes), rounds it to bf16 and  */
  /* uses it as the K-extension operand -- the separate skinny pass over A disappears.  The tiles of column   */
  /* 0 also write T [M,Rp] and, if non-NULL, Tt [Rp,ldt] (for cara_tskinny_*).                                */
  const void* Ut;
  void* T_out;
  void* Tt_out;
  int ldt;
  /* Optional second image of B in K-PANEL-MAJOR layout (cara_pack_b_panels): bf16 [K/32][N][32], i.e. the 32     */
  /* columns of K step t of ALL rows are contiguous, so the 128 x 32 operand tile of a K step is one 8-KiB run of  */
  /* full cache lines instead of 128 half lines 2*ldb bytes apart (the L2 -> LDS path delivers ~30 % more tile     */
  /* bytes per second that way, tools/micro/kloop_bw.hip).  Frozen weights are packed once at ingest.  The 32-     */
  /* GEMM reads it INSTEAD of B when non-NULL (B is then only used by the few-row path).                      */
  const void* Bp;
  /* Activations in the same K-panel-major layout (bf16 only; M > 128, no batch).                                    */
  /* a_panels = P > 0: A is [K/32][P][32] (P >= M rows per panel), lda is ignored.      */
  /* c_panels = P > 0 (bf16 epilogues): C is WRITTEN as [N/32][P][32] -- the A operand of the next GEMM, the X of   */
  /* cara_skinny_xu / cara_tskinny_* with ldx = -P -- while C2 / aux keep the row-major ldc.  N % 32 == 0 then.     */
  int a_panels, c_panels;
  /* Optional SECOND B operand, same shape and ldb as B (row-major, bf16): C = A B^T + A B3^T (+ the K-extension), the two  */
  /* products accumulated in fp32 in ONE launch (the K loop runs over B, then over B3).  For a small correction to a large   */
  /* operand -- the exact weight-dropout mode's masked adapter delta against the frozen weight -- that a pre-merged bf16      */
  /* B + B3 would round away.  Plain product only: no Bp, batch, Ut, a_panels or tskinny with it.                            */
  const void* B3;
  /* With Ut: the adapter's rank, if the caller knows it (0 = not stated).  At Rp = 32 and 1 <= Ut_rank <= 16 the kernel computes  */
  /* columns 0 .. 15 of T only (rows >= rank of Ut are zero) and writes columns 16 .. 31 as zeros: same results, bit for bit.      */
  int Ut_rank;
  /* Epilogue riders (CARA_EPI_MULH only; er_Tt == NULL: none).  The tile that has just produced dH = acc * gelu'(u) holds half of what  */
  /* two transposed skinny products of the backward need: dVs = dH^T T of the linear whose dY this C is (fc1), and dU = h^T G' of this    */
  /* linear (fc2) with the h = gelu(u) tile at the same coordinates (er_h: bf16, row-major with C's ldc, or K-panel-major                 */
  /* [N/32][er_h_panels][32]) -- read here once, 16 bytes per lane, instead of 77 MB of dH and 77 MB of h re-read per block by products   */
  /* that ride in the next launch.  Every workgroup multiplies its bf16 dH / h tile, transposed through LDS, by its rows of er_Tt / er_Gt */
  /* (bf16 [>= 16, er_ldg]: T^T and G'^T, rows = the first 16 adapter columns, er_ldg >= M) and writes 16-wide fp32 partial sums for its   */
  /* 128 columns: slab `row tile` of column block n / 64, in the layout of cara_tskinny_partial2_r at rank <= 16 with                     */
  /* cara_gemm_epi_rider_chunks(a) slabs per column block (er_colsum: column sums of dH behind the er_slabs_v slabs, as want_colsum       */
  /* leaves them).  Reduce with cara_ts_reduce::Rc = 16, ::wave_slabs = that chunk count.  Each slab region:                              */
  /* cara_gemm_epi_rider_scratch_bytes(chunks, N).                                                                                         */
  const void* er_Tt;
  const void* er_Gt;
  const void* er_h;
  void* er_slabs_v;
  void* er_slabs_u;
  int er_ldg, er_colsum, er_h_panels;
} cara_gemm_args;
int cara_gemm_bf16(const cara_gemm_args* a, void* stream);
/* Slabs per column block a launch of `a` with epilogue riders writes (= its row tiles), 0: this product cannot carry them (then  */
/* cara_gemm_bf16 / cara_gemm_with_tskinny* return CARA_E_ARG when er_Tt is set).  Needs CARA_EPI_MULH, M > 1024, N >= 3072,      */
/* N % 128 == 0, ldc % 8 == 0, no batch, M % 4 == 0.  Depends on the arguments only.                                              */
int cara_gemm_epi_rider_chunks(const cara_gemm_args* a);
/* The same fields with CARA_EPI_BF16 (er_h NULL, er_Gt / er_slabs_u unused): the dX GEMM of a linear stages that linear's dY as its A   */
/* operand, so its K loop can leave dVs = A^T T (+ the column sums of A with er_colsum) on the way -- from the A tiles in LDS, nothing is */
/* read again.  Slab (row tile of 160, K step of 64) of er_slabs_v, the layout above with K in the place of N; only on the 160 x 256 x 64 */
/* tile: cara_gemm_dv_chunks(a, riders) = the slabs per column block such a launch writes (riders: it also carries a product through      */
/* cara_gemm_with_tskinny_r), 0 = this product cannot (cara_gemm_bf16 then returns CARA_E_ARG).  A K-extension is required (A2 or Ut).    */
int cara_gemm_dv_chunks(const cara_gemm_args* a, int riders);
size_t cara_gemm_epi_rider_scratch_bytes(int chunks, int N);
/* B bf16 [N, K] (row stride ldb) -> out bf16 [K/32][N][32] (cara_gemm_args::Bp); K % 32 == 0 */
int cara_pack_b_panels(const void* B, int ldb, int N, int K, void* out, void* stream);
size_t cara_gemm_scratch_bytes(void);

/* C[z] fp32 [M, ldc] = sum over the rows k of slab z of At[k, m] * Bt[k, n], z = 0 .. nslab - 1, slab z at C + z * slab_stride
 * floats (rows [z * kslab, (z + 1) * kslab) with kslab = K / nslab rounded up to 32).  At bf16 [K, lda >= M], Bt bf16
 * [K, ldb >= N], both ROW-major with the shared index k on the rows: dW = dY^T X (the dense weight gradient of the exact
 * weight-dropout mode) from the activations as they are stored, without transposed copies.  M % 128 == N % 128 == 0,
 * ld % 8 == 0, each operand < 4 GiB; CARA_E_ARG otherwise (callers then transpose and use cara_gemm_bf16).       */
int cara_gemm_tn_f32(const void* At, int lda, const void* Bt, int ldb, float* C, int ldc, int M, int N, int K, int nslab,
                     size_t slab_stride, void* stream);

/* ---- skinny adapter contractions (HBM-bound) --------------------------------------------- */
/* T[M,Rp] = X[M,K] * Ut[Rp,K]^T, bf16 out, also written transposed Tt[Rp,ldt] when Tt != NULL
 * (ldt >= M, multiple of 8).  Forward: T = X U; backward: G' = dY Vs.  K % 32 == 0.
 * In this function and in cara_tskinny_*, a NEGATIVE ldx says that X is K-panel-major: bf16 [K/32][-ldx][32]
 * with -ldx >= M rows per panel (what a GEMM with cara_gemm_args::c_panels = -ldx wrote).                  */
int cara_skinny_xu(const void* X, int ldx, const void* Ut, void* T, void* Tt, int ldt,
                   int M, int K, int Rp, void* stream);
/* The same with the adapter's rank stated (1 <= rank <= Rp; rows >= rank of Ut are zero): at Rp = 32 and rank <= 16 only the
 * first 16 columns are computed (half the Ut fragments and MFMAs of a pass that is bound by what a workgroup pays once) and
 * columns 16 .. 31 of T / rows 16 .. 31 of Tt are written as the zeros they are.  Same results, bit for bit.          */
int cara_skinny_xu_r(const void* X, int ldx, const void* Ut, void* T, void* Tt, int ldt,
                     int M, int K, int Rp, int rank, void* stream);
/* D[K1,Rp] (fp32) = sum_m X[m,K1] * G[m,Rp]  given Gt[Rp,ldg] (= G transposed, bf16); optional
 * colsum[K1] (fp32) = sum_m X[m,:].  Outputs are OVERWRITTEN.  `slabs` is caller scratch of
 * cara_tskinny_scratch_bytes(M, K1, Rp) bytes.  Gives dU = X^T G' and dVs = dY^T T (A.4).      */
size_t cara_tskinny_scratch_bytes(int M, int K1, int Rp);
int cara_tskinny_xtg(const void* X, int ldx, const void* Gt, int ldg, float* D, float* colsum,
                     void* slabs, int M, int K1, int Rp, void* stream);
/* The same in two steps, so that the tiny fixed-order slab sums of many products (the 12 layers
 * of one linear) run as ONE launch: _partial writes the per-block slabs of one product into its
 * own scratch region; _reduce sums `batch` regions spaced slab_stride bytes apart into
 * D[batch,K1,Rp] (and colsum[batch,K1] when non-NULL; every region must then hold column sums). */
int cara_tskinny_partial(const void* X, int ldx, const void* Gt, int ldg, void* slabs, int want_colsum,
                         int M, int K1, int Rp, void* stream);
/* Two products in ONE launch (the dU = X^T G' and dVs = dY^T T of one linear; both Gt share ldg
 * and M; only the second may ask for column sums).                                             */
int cara_tskinny_partial2(const void* Xa, int ldxa, const void* Gta, void* slabs_a, int K1a,
                          const void* Xb, int ldxb, const void* Gtb, void* slabs_b, int K1b, int want_colsum_b,
                          int ldg, int M, int Rp, void* stream);
/* cara_gemm_bf16(a) and cara_tskinny_partial2(...) of the SAME linear as ONE launch: the grid holds the GEMM's tiles
 * and the products' blocks, so the HBM-bound products run under the MFMA-bound GEMM without a second stream (no
 * event between the kernels before and after).  M > 128, no batch; Rp in {32, 64} (64: three workgroups per CU); the
 * products need not be those of the GEMM's own linear (their M may differ from a->M); with a->Ut (the adapter inside
 * the GEMM) only CARA_EPI_BF16 and products of the same Rp.  CARA_E_ARG otherwise (callers then launch the two
 * separately).  The GEMM's epilogue: CARA_EPI_BF16, CARA_EPI_DGELU or CARA_EPI_MULH (the dX products).  Results are bitwise
 * those of the two calls.                                                                                          */
int cara_gemm_with_tskinny(const cara_gemm_args* a, const void* Xa, int ldxa, const void* Gta, void* slabs_a, int K1a,
                           const void* Xb, int ldxb, const void* Gtb, void* slabs_b, int K1b, int want_colsum_b,
                           int ldg, int M, int Rp, void* stream);
int cara_tskinny_reduce(const void* slabs, size_t slab_stride, float* D, float* colsum, int batch,
                        int M, int K1, int Rp, void* stream);
/* cara_tskinny_partial2 / cara_gemm_with_tskinny with the adapter's rank stated (1 <= rank <= Rp): at Rp = 32 and rank <= 16
 * the products compute the first 16 of their 32 columns only (the others are zero by construction: rows >= rank of Gt are
 * zero) and write 16-WIDE slabs -- reduce them with cara_ts_reduce::Rc = 16 (cara_tskinny_reduce_many), which sums those
 * columns and writes the other columns of D as zeros.  Otherwise identical to the functions without _r.                  */
int cara_tskinny_partial2_r(const void* Xa, int ldxa, const void* Gta, void* slabs_a, int K1a,
                            const void* Xb, int ldxb, const void* Gtb, void* slabs_b, int K1b, int want_colsum_b,
                            int ldg, int M, int Rp, int rank, void* stream);
int cara_gemm_with_tskinny_r(const cara_gemm_args* a, const void* Xa, int ldxa, const void* Gta, void* slabs_a, int K1a,
                             const void* Xb, int ldxb, const void* Gtb, void* slabs_b, int K1b, int want_colsum_b,
                             int ldg, int M, int Rp, int rank, void* stream);
/* How the products that ride in cara_gemm_with_tskinny_r(a, ..., Rp, rank, ...) leave their partial sums: 0 = one slab per block
 * (every other entry point of this section), 1 = one slab per WAVE, four per block -- the long-K, narrow-N dX products run on a
 * 160 x 256 x 64 tile, one workgroup per CU, whose riding products are streamed by helper waves UNDER the tile's K loop: a helper
 * wave owns one wave's steps of a block and writes its own slab (no combine through LDS).  Pass the answer as
 * cara_ts_reduce::wave_slabs.  cara_tskinny_scratch_bytes() covers both forms.  Depends on the arguments only.            */
int cara_gemm_rider_slab_format(const cara_gemm_args* a, int Rp, int rank);
/* Up to CARA_TS_REDUCE_MAX of those reductions in ONE launch (each entry = the arguments of cara_tskinny_reduce). */
#define CARA_TS_REDUCE_MAX 24
typedef struct {
  const void* slabs; size_t slab_stride; float* D; float* colsum;   /* colsum may be NULL; slabs, D, slab_stride: multiples of 16 bytes */
  int batch, M, K1, Rp;
  int Rc;   /* columns the slabs hold: 0 or Rp = all; 16 (at Rp = 32) = slabs written by the _r functions at rank <= 16 */
  int wave_slabs;   /* 1: the product wrote one slab per WAVE of its blocks (four per block): what cara_gemm_with_tskinny_r does  */
                    /* where cara_gemm_rider_slab_format() says so; 0: one slab per block; >= 2: that many slabs per column      */
                    /* block (the epilogue riders of cara_gemm_args::er_*: cara_gemm_epi_rider_chunks)                            */
} cara_ts_reduce;
int cara_tskinny_reduce_many(const cara_ts_reduce* probs, int n, void* stream);

/* ---- one adapted linear per call (cara_linear_fwd / cara_linear_bwd) -------------------------------- */
/* The adapter linear of cara.py:25-42 (qkv), :50-58 (proj), :75-82 (fc1), :87-93 (fc2) in factored form as ONE call each way:
 * compositions of the entry points above, for an integrator who patches one nn.Linear at a time (cara_vit_forward /
 * cara_vit_backward schedule the same pieces with more fusion).  The per-layer factor images come from cara_factor_prep:
 * Ut [Rp, in] = U^T, U [in, Rp], Vs [out, Rp] = s g (.) V, Vst [Rp, out] (bf16, columns / rows >= rank zero), bias = b + s c.  */
typedef struct {
  const void* W;  const void* Wt;     /* bf16 [out, in] frozen weight; [in, out] its transpose (backward only)             */
  const void* Ut; const void* U;      /* bf16 [Rp, in], [in, Rp]                                                           */
  const void* Vs; const void* Vst;    /* bf16 [out, Rp], [Rp, out]                                                         */
  const float* bias;                  /* fp32 [out] or NULL                                                                */
  int in, out, Rp, rank;              /* Rp in {32, 64}, 1 <= rank <= Rp                                                   */
} cara_linear;
/* Y = epilogue(X W^T + bias + (X U) Vs^T): T [M, Rp] = X U (bf16) and its transpose Tt [Rp, ldt] (ldt >= M rounded up to 32,
 * multiple of 8) are WRITTEN -- the backward reads Tt.  epi / Y / Y2 / aux / rowscale / rows_per_sample: the epilogue fields of
 * cara_gemm_args -- C, C2, aux, ...; ldy = 0: dense.  X bf16 [M, ldx].                                                     */
int cara_linear_fwd(const cara_linear* L, const void* X, int ldx, int M, void* T, void* Tt, int ldt, int epi, void* Y, int ldy,
                    void* Y2, const void* aux, const float* rowscale, int rows_per_sample, void* stream);
/* Given dY bf16 [M, lddy], the saved input X and the forward's Tt: G [M, Rp] = dY Vs and Gt (scratch, written);
 * dX bf16 [M, lddx] = dY W + G U^T (skipped when NULL); dU fp32 [in, Rp] = X^T G, dVs fp32 [out, Rp] = dY^T T, dc fp32 [out] =
 * column sums of dY (NULL: not wanted) -- the gradients cara_factor_grad_reduce takes per layer.  slabs_u / slabs_v:
 * cara_tskinny_scratch_bytes(M, in, Rp) / (M, out, Rp) bytes of caller scratch; they, dU and dVs: 16-byte aligned.         */
int cara_linear_bwd(const cara_linear* L, const void* dY, int lddy, const void* X, int ldx, const void* Tt, int M, void* G, void* Gt,
                    int ldt, void* dX, int lddx, void* slabs_u, void* slabs_v, float* dU, float* dVs, float* dc, void* stream);

/* ---- LayerNorm (eps inside the sqrt, biased variance; timm Block norm1/norm2/norm) ------- */
/* y bf16 [M,C] = (x - mean) * rstd * gamma + beta; saves mean, rstd fp32 [M].  x fp32 rows with
 * stride ldx elements (ldx = tokens*C picks the cls rows for the final norm).  C % 256 == 0.   */
int cara_layernorm_fwd(const float* x, long ldx, const float* gamma, const float* beta, void* y,
                       float* mean, float* rstd, int M, int C, float eps, void* stream);
/* dx_out fp32 = dx_in + LN'(dy) ; optional dyb bf16 = rowscale[m / rows_per_sample] * dx_out.
 * dy is bf16 [M,C]; x/dx rows strided by ldx like the forward.  dx_in may be NULL (= 0) and may
 * alias dx_out.                                                                               */
int cara_layernorm_bwd(const void* dy, const float* x, long ldx, const float* gamma,
                       const float* mean, const float* rstd, const float* dx_in, float* dx_out,
                       void* dyb, const float* rowscale, int rows_per_sample, int M, int C,
                       void* stream);
/* The same with the skinny adapter product of the NEXT linear fused in (its input row is in registers
 * here, so the separate cara_skinny_xu pass and its re-read of the activations disappear):
 *   _fwd_xu: T[M,Rp] = y Ut^T (Ut bf16 [Rp,C], rows >= rank zero), Tt[Rp,ldt] its transpose (or NULL);
 *   _bwd_xu: G[M,Rp] = dyb Vst^T with dyb the row-scaled bf16 gradient this kernel emits (dyb may be NULL
 *            when only G is wanted), Gt its transpose.  Same rounding points as cara_skinny_xu.
 * Rp in {32, 64} (rank <= Rp), C in {256, 768, 1024}; else CARA_E_ARG (callers then keep the separate
 * cara_skinny_xu pass).                                                                                  */
int cara_layernorm_fwd_xu(const float* x, long ldx, const float* gamma, const float* beta, void* y,
                          float* mean, float* rstd, int M, int C, float eps, const void* Ut, int rank,
                          int Rp, void* T, void* Tt, int ldt, void* stream);
int cara_layernorm_bwd_xu(const void* dy, const float* x, long ldx, const float* gamma,
                          const float* mean, const float* rstd, const float* dx_in, float* dx_out,
                          void* dyb, const float* rowscale, int rows_per_sample, int M, int C,
                          const void* Vst, int rank, int Rp, void* G, void* Gt, int ldt, void* stream);
/* The general forms: Ut / Vst may be NULL (no fused product), and the bf16 output (y, resp. dyb) is written
 * K-panel-major -- [C/32][panels][32] with panels >= M rows per panel, the layout cara_gemm_args::a_panels
 * and a negative ldx of the skinny products read -- when y_panels / dyb_panels > 0 (0 = row-major).        */
int cara_layernorm_fwd_ex(const float* x, long ldx, const float* gamma, const float* beta, void* y,
                          float* mean, float* rstd, int M, int C, float eps, const void* Ut, int rank,
                          int Rp, void* T, void* Tt, int ldt, int y_panels, void* stream);
int cara_layernorm_bwd_ex(const void* dy, const float* x, long ldx, const float* gamma,
                          const float* mean, const float* rstd, const float* dx_in, float* dx_out,
                          void* dyb, const float* rowscale, int rows_per_sample, int M, int C,
                          const void* Vst, int rank, int Rp, void* G, void* Gt, int ldt, int dyb_panels,
                          void* stream);

/* ---- attention (cara.py:43-48; softmax(q k^T * scale) v per head) ------------------------- */
/* qkv bf16 [B*N, 3*H*64] with column k*H*64 + h*64 + d (k = q,k,v): exactly the layout
 * cara.py:39 reshapes.  out bf16 [B*N, H*64]; lse fp32 [B,H,N].  Head dim 64; N <= 2^20 and      *
 * B*N < 2^31 (index arithmetic; no limit from LDS).  N <= 224: score rows in registers; N <= 608:  *
 * two sweeps over the key tiles, whole K/V of a head in LDS; above (and for 224 < N <= 608 with    *
 * CARA_ATTN_STREAM=1): the same two sweeps with K/V (backward: also Q/dO) streamed through LDS in   *
 * 64-row tiles.  No atomics on any path: results are bitwise reproducible.                         */
int cara_attention_fwd(const void* qkv, void* out, float* lse, int B, int N, int H, float scale,
                       void* stream);
int cara_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse,
                       void* dqkv, int B, int N, int H, float scale, void* stream);
/* The same for the cls query alone (row 0 of every sample) -- all the LAST block needs: only the cls row of its attention
 * output reaches the logits (timm's `x[:, 0]` behind the final norm; cara.py:43-48 computes every row).  _fwd writes
 * out[b N + 0, :] and lse[b, h, 0] and leaves the other rows alone; _bwd reads those rows (and dout[b N + 0, :]) and writes
 * ALL of dqkv: dK / dV of every key row, dQ of the cls row, zeros for the dQ of the other rows.  Same rounding points as the
 * full kernels.  N as for the full kernels (above 608 tokens _fwd sweeps the keys twice instead of keeping the score row in LDS). */
int cara_attention_cls_fwd(const void* qkv, void* out, float* lse, int B, int N, int H, float scale, void* stream);
int cara_attention_cls_bwd(const void* qkv, const void* out, const void* dout, const float* lse,
                           void* dqkv, int B, int N, int H, float scale, void* stream);

/* ---- small pieces of the ViT around the blocks -------------------------------------------- */
/* patches bf16 [B*gh*gw, C*p*p] <- images fp32 [B,C,Hi,Wi]  (Conv2d k=s=p as a GEMM operand)  */
int cara_im2col_patches(const float* img, void* patches, int B, int C, int Hi, int Wi, int p,
                        void* stream);
/* The same patch rows straight from uint8 pixels [B,C,Hi,Wi] (a resident data split): ToTensor + Normalize of
 * vtab.py:92-94 per element in fp32, in this order -- u / 255, - mean[c], / std[c], both divisions correctly rounded --
 * then the one rounding to the build's 16-bit type.  mean / std: device fp32 [C].  pixels 4-byte aligned.  The fp32
 * image is never written; the rows are bitwise those of cara_im2col_patches on the fp32 image so computed.          */
int cara_im2col_patches_u8(const unsigned char* pixels, const float* mean, const float* std, void* patches,
                           int B, int C, int Hi, int Wi, int p, void* stream);
/* cara_im2col_patches_u8 over rows of a whole resident split: pixels uint8 [n_split,C,Hi,Wi], rows device int64 [B] (any
 * order, duplicates allowed); the patch rows of sample i come from image rows[i], same arithmetic and rounding points.  An
 * index outside [0, n_split) is never dereferenced: that sample's patch rows are zeros and *bad (device int, may be NULL;
 * the caller clears it) is incremented once per such sample.                                                            */
int cara_im2col_patches_u8_rows(const unsigned char* pixels, int n_split, const int64_t* rows, const float* mean,
                                const float* std, void* patches, int* bad, int B, int C, int Hi, int Wi, int p, void* stream);
/* cara_im2col_patches_u8_rows through a crop box per sample (random-resized crop and flip by index): pixels uint8
 * [n_split,C,Hs,Ws] -- any size, not the model's, Ws need not be a multiple of 4, no alignment asked -- and boxes device int32
 * [B,5] = (x0, y0, w, h, flip) in source pixels.  Output pixel (oy, ox) of sample b, channel c, in fp32:
 *   ox' = flip ? Wi-1-ox : ox;  sx = max((ox' + 0.5) * (w / Wi) - 0.5, 0);  ix0 = min((int)sx, w-1);  ix1 = min(ix0+1, w-1);
 *   fx = sx - ix0;  the same for y with h / Hi;  v = (1-fy) ((1-fx) u00 + fx u01) + fy ((1-fx) u10 + fx u11)
 * on the bytes at (y0+iy*, x0+ix*) of image rows[b], each axis evaluated as a + f (b - a) (exact where f == 0 or a == b); then
 * (v / 255 - mean[c]) / std[c] and the one rounding to the build's 16-bit type, as in cara_im2col_patches_u8.  That is bilinear
 * interpolate(align_corners = false, no antialias filter) of the box followed by a horizontal flip; indices are clamped inside
 * the box.  A box of the output's size gives bit for bit the patch rows of cara_im2col_patches_u8 on those bytes.  A row
 * outside [0, n_split) or a box not inside the source (w < 1, h < 1, x0 < 0, y0 < 0, x0+w > Ws, y0+h > Hs) is never
 * dereferenced: zero patch rows, *bad (may be NULL) incremented once per such sample.  flip: non-zero means flip.        */
int cara_im2col_patches_u8_rows_crop(const unsigned char* pixels, int n_split, int Hs, int Ws, const int64_t* rows,
                                     const int* boxes, const float* mean, const float* std, void* patches, int* bad, int B,
                                     int C, int Hi, int Wi, int p, void* stream);
/* cara_im2col_patches_u8_rows_crop with Mixup / CutMix by index: mix device int32 [B,8], row b = (partner, cx0, cy0, cw, ch,
 * blend, target, 0).  partner in [0, B) (b itself allowed): the sample whose UNMIXED value at the same output position -- through
 * rows[partner] and boxes[partner], its flip included -- is mixed in.  (cx0, cy0, cw, ch): the CutMix rectangle in output pixels;
 * inside it the pixel is the partner's; cw == 0 or ch == 0: no rectangle.  blend: the bits of an fp32 m in [0, 1]; outside the
 * rectangle the pixel is a + m (b - a) in fp32 on the un-normalised 0..255 values (a the sample's own bilinear value, b the
 * partner's; exact at m == 0), then (v / 255 - mean[c]) / std[c] and the one rounding to 16 bits.  target: the bits of an fp32 t,
 * the weight of the partner's label -- read by cara_cross_entropy_mix only.  The last word is written as 0 and not read.
 * boxes may be NULL: every sample reads its whole image, and Hs == Hi, Ws == Wi is asked.  A sample gets zero patch rows and
 * is counted once in *bad (may be NULL) when its own or its partner's row or box is bad (by the rules above), its partner is
 * outside [0, B), its rectangle is not inside the output (cx0, cy0, cw, ch >= 0, cx0+cw <= Wi, cy0+ch <= Hi) or its m is not in
 * [0, 1] (a NaN is not); none of these values is used before it is checked.  An identity table (partner = b, the rest 0)
 * gives bit for bit the patch rows of cara_im2col_patches_u8_rows_crop, or of cara_im2col_patches_u8_rows without boxes.  */
int cara_im2col_patches_u8_rows_mix(const unsigned char* pixels, int n_split, int Hs, int Ws, const int64_t* rows,
                                    const int* boxes, const int* mix, const float* mean, const float* std, void* patches,
                                    int* bad, int B, int C, int Hi, int Wi, int p, void* stream);
/* cara_im2col_patches_u8_rows_mix with colour jitter and Random Erasing by index: aug device int32 [B,16], row b =
 *   (op0, f0, op1, f1, op2, f2, ex0, ey0, ew, eh, emode, eseed, 0, 0, 0, 0)
 * op: 0 none, 1 brightness, 2 contrast, 3 saturation -- a non-zero code at most once per row, in any order; f: the bits of a finite
 * fp32 factor >= 0 (not read where op == 0); (ex0, ey0, ew, eh): the erase rectangle in output pixels, ew == 0 or eh == 0: none;
 * emode: 0 const, 1 pixel; eseed: any 32 bits; the last four words 0.  All of it in fp32, every product and sum one IEEE operation
 * (no contraction), on the un-normalised 0..255 values; u = the sample's own unmixed bilinear value (as above):
 *   each slot in order:  v <- min(max(f v + (1 - f) d, 0), 255), 1 - f rounded once;  brightness d = 0;  saturation d = gray =
 *   (0.2989 r + 0.587 g) + 0.114 b of that pixel's three channel values at that point of the chain;  contrast d = M_b, the mean of gray
 *   over all Hi x Wi output pixels of sample b as they stand before the contrast slot (torchvision's _blend on float tensors,
 *   rescaled to 0..255: exact at f == 1, d clamped at f == 0).  M_b comes from a pre-pass through a fixed tree: 16 workgroups of 256
 *   threads per sample; thread t of workgroup k adds gray of the pixels q = 256 k + t, + 4096, ... < Hi Wi (q = oy Wi + ox) in
 *   sequence; the wave's 64 sums by a butterfly (lanes 32, 16, 8, 4, 2, 1 apart); the four wave sums left to right; the 16 workgroup
 *   sums left to right; one division by (float)(Hi Wi).
 *   Then the mix step exactly as in cara_im2col_patches_u8_rows_mix, the partner's value being the partner's unmixed value after its
 *   own chain (its row of aug, its M); then (v / 255 - mean[c]) / std[c]; then the erase: inside the rectangle the normalised value
 *   becomes 0 (const) or z (pixel):  i = ((b C + c) Hi + oy) Wi + ox;  h1 = cara_weight_dropout_hash(2 i, eseed, 0x45524153), h2 =
 *   ...(2 i + 1, ...);  u1 = ((h1 >> 8) + 1) 2^-24 in (0, 1], u2 = (h2 >> 8) 2^-24 in [0, 1) (exact);
 *   z = sqrtf(-2 logf(u1)) cosf(6.2831855f u2) -- roundings: logf, sqrtf, the product 6.2831855f u2, cosf, the last product (the
 *   product with -2 is exact);  then the one rounding to the build's 16-bit type.
 * mix and boxes may each be NULL (no partner; whole images, Hs == Hi and Ws == Wi asked).  aug NULL: the call without a table
 * (the launches of _rows_mix, _rows_crop or _rows).  stat_scratch: cara_aug_stat_bytes(B) bytes of device memory, 4-byte aligned
 * (fp32 stat [B], then the tree's partial sums); a sample without a contrast op loads no pixel in the pre-pass and its stat word
 * is neither written nor read.  C must be 3 and 2 B C Hi Wi <= 2^32: CARA_E_ARG otherwise, nothing launched.  A sample gets zero
 * patch rows and is counted once in *bad by the rules of _rows_mix and where its own OR ITS PARTNER's aug row has an op outside
 * [0, 3], a repeated op, a factor that is negative, infinite or NaN, a rectangle not inside the output (ew, eh, ex0, ey0 >= 0, ew <=
 * Wi - ex0, eh <= Hi - ey0, in this order), an emode outside {0, 1} or a non-zero pad word.  An all-zero aug table gives bit for bit
 * the patch rows of the call without it.                                                                                        */
size_t cara_aug_stat_bytes(int B);
int cara_im2col_patches_u8_rows_aug(const unsigned char* pixels, int n_split, int Hs, int Ws, const int64_t* rows,
                                    const int* boxes, const int* mix, const int* aug, void* stat_scratch, const float* mean,
                                    const float* std, void* patches, int* bad, int B, int C, int Hi, int Wi, int p, void* stream);
/* Patch dropout (timm's PatchDropout): the patch rows of a kept subset only.  keep device int32 [B,K], 1 <= K <= P = (Hi/p) (Wi/p),
 * entries in [0, P) (patch index gy (Wi/p) + gx), any order; the host refuses duplicates within a sample, the device does not look.
 * Output row b K + j is the patch row of patch keep[b][j] of sample b: patches bf16 [B*K, C*p*p].  Everything a row holds is a
 * function of its pixels' positions in the FULL Hi x Wi output image, so a kept row is bit for bit the row of the same patch that
 * the call without keep writes -- cara_im2col_patches for the first entry; for the second cara_im2col_patches_u8_rows_aug with the
 * same tables, each of boxes / mix / aug NULL or not under that entry's rules (the contrast pre-pass is that entry's, unchanged: it
 * still reduces the whole image; the erase noise keeps its element index i in [B,C,Hi,Wi]).  A keep entry outside [0, P) is never
 * used as an index: its row is zeros and *bad (may be NULL) is incremented once per such entry.  A sample that the rules above call
 * bad (row, box, mix or aug entry) gets K zero rows and is counted once; its keep entries are not counted again.                  */
int cara_im2col_patches_keep(const float* img, const int* keep, int K, void* patches, int* bad, int B, int C, int Hi, int Wi,
                             int p, void* stream);
int cara_im2col_patches_u8_rows_keep(const unsigned char* pixels, int n_split, int Hs, int Ws, const int64_t* rows,
                                     const int* boxes, const int* mix, const int* aug, void* stat_scratch, const int* keep, int K,
                                     const float* mean, const float* std, void* patches, int* bad, int B, int C, int Hi, int Wi,
                                     int p, void* stream);
/* RandAugment by index: cara_im2col_patches_u8_rows_keep / _aug with one more device table, ra int32 [B,16], row b =
 *   (op0, arg0, op1, arg1, op2, arg2, m00, m01, m02, m10, m11, m12, fill, 0, 0, 0)
 * op: a lookup slot on the quantised value q, applied in the order 0, 1, 2 -- 0 none (arg 0); 1 posterize, arg = bits kept 0..8:
 * q & ~((1 << (8 - arg)) - 1); 2 solarize, arg = threshold 0..256: q < arg ? q : 255 - q; 3 solarize-add, arg 0..255: q < 128 ?
 * min(q + arg, 255) : q; 4 invert: 255 - q (arg 0); 5 autocontrast, 6 equalize (arg 0; at most one of the two per row).  m..: the
 * bits of six finite fp32 numbers of magnitude <= 32768, the output-to-input affine; fill = 0x00RRGGBB.  All of it in fp32, every
 * product and sum one IEEE operation (no contraction).  Output pixel (ox, oy), x = ox + 0.5, y = oy + 0.5:
 *   u = (m00 x + m01 y) + m02, v = (m10 x + m11 y) + m12; unless 0 <= u < Wi and 0 <= v < Hi the value is the channel's fill byte;
 *   inside, the sample's box (w x h, flip) at the continuous position: uf = flip ? Wi - u : u, s = max(uf (w / Wi) - 0.5, 0), i0 =
 *   min((int)s, w - 1), i1 = min(i0 + 1, w - 1), f = s - i0; the same for v with h / Hi and no flip; t + fy (b - t) of the two rows'
 *   a + f (b - a).  A row whose matrix words are the bits of (1, 0, 0, 0, 1, 0) gives bit for bit the value of the call without ra.
 *   With any lookup slot: q = (int)rintf(value) (half to even), the slots, (float)q -- the fill pixels too; without: no quantising.
 *   Then the chain of the aug row (its contrast mean M_b is taken over these values), the mix (the partner's value after its own
 *   ra row, tables and aug row), the normalisation, the erase and the one rounding, as in cara_im2col_patches_u8_rows_aug.
 * Statistic slot: h_c[256] = the histogram of q as it stands before that slot over all Hi x Wi output pixels of channel c (fill
 * pixels count; keep does not change it).  autocontrast: lo, hi = first / last non-zero bin; hi <= lo: identity; else lut[i] =
 * clamp((255 (i - lo)) / (hi - lo), 0, 255), integer division, 0 below lo.  equalize: z = h[hi], step = (sum h - z) / 255; hi <= lo
 * or step == 0: identity; else lut[i] = min(255, (step / 2 + sum_{j<i} h[j]) / step).  Pre-pass: 8 workgroups per sample count
 * into LDS with integer atomics and store their partial histograms; one workgroup per (sample, channel) sums them and writes the
 * table.  ra_scratch: cara_ra_stat_bytes(B) bytes, 4-byte aligned (uint8 lut [B][3][256], then int32 partial [B][8][3][256]); what
 * it held before the call does not matter; a sample without a statistic slot loads no pixel in the pre-pass.
 * Every table but rows may be NULL (keep NULL: all rows, K ignored).  ra NULL: the launches of _rows_keep / _rows_aug.  With ra, C
 * must be 3 and ra_scratch present: CARA_E_ARG otherwise, nothing launched.  A sample gets zero patch rows and is counted once in
 * *bad by the rules above and where its own OR ITS PARTNER's ra row has an op outside [0, 6], an argument outside its range, two
 * statistic slots, a matrix word that is not finite or above 32768 in magnitude, a fill above 0xFFFFFF or a non-zero pad word.      */
size_t cara_ra_stat_bytes(int B);
int cara_im2col_patches_u8_rows_ra(const unsigned char* pixels, int n_split, int Hs, int Ws, const int64_t* rows, const int* boxes,
                                   const int* mix, const int* aug, void* stat_scratch, const int* ra, void* ra_scratch,
                                   const int* keep, int K, const float* mean, const float* std, void* patches, int* bad, int B,
                                   int C, int Hi, int Wi, int p, void* stream);
/* out[i] = labels[rows[i]] (device int64 [B] each; labels int64 [n_split]); a row outside [0, n_split) is not
 * dereferenced: it gives 0 and is counted in *bad (device int, may be NULL)                                    */
int cara_gather_labels(const int64_t* labels, int n_split, const int64_t* rows, int64_t* out, int B, int* bad,
                       void* stream);
/* x fp32 [B,1+P,D]: row 0 = cls + pos[0]; row 1+i = emb[b*P+i] + pos[1+i]                      */
int cara_assemble_tokens(const float* emb, const float* cls, const float* pos, float* x, int B,
                         int P, int D, void* stream);
/* cara_assemble_tokens behind a patch dropout: emb fp32 [B*K, D] holds the kept patches' embeddings (row b K + j = patch keep[b][j]),
 * pos fp32 [1+P, D] the full position embedding.  x fp32 [B,1+K,D]: row 0 = cls + pos[0]; row 1+j = emb[b*K+j] + pos[1 + keep[b][j]],
 * one fp32 add -- with keep[b][j] = j and K == P bit for bit cara_assemble_tokens.  For an entry outside [0, P) pos is not
 * dereferenced and the row is emb's alone.  (P is an argument because the range of keep is not otherwise known here.)              */
int cara_assemble_tokens_keep(const float* emb, const float* cls, const float* pos, const int* keep, float* x, int B, int K,
                              int P, int D, void* stream);
/* loss[0] = mean cross-entropy over B (loss must hold 1 + B floats: [1..B] is scratch);
 * dlogits (optional) = (softmax - onehot)/B ; logits fp32 [B,C]   (vit_cp.py:47)
 * A label outside [0, C) is never used as an index: that sample's term loss[1 + b], its dlogits row and loss[0] are NaN. */
int cara_cross_entropy(const float* logits, const int64_t* labels, float* loss, float* dlogits,
                       int B, int C, void* stream);
/* The same with the gradient pre-scaled, so that a train step needs no separate scaling launches:
 *   dlogits = (softmax - onehot)/B * dscale * (loss_scale ? *loss_scale : 1)
 * dscale (host) = 1/world_size of a data-parallel job (the all-reduce is then a plain SUM); loss_scale (device float,
 * may be NULL) = the dynamic loss scale of the IEEE-half operand build (cara_amp_update).  found_inf (device float, may
 * be NULL) is set to 0 here: the backward's final gradient writes raise it (cara_vit_shape::found_inf).  loss[0] is the
 * UNSCALED mean loss.                                                                                                  */
int cara_cross_entropy_ex(const float* logits, const int64_t* labels, float* loss, float* dlogits,
                          int B, int C, float dscale, const float* loss_scale, float* found_inf, void* stream);
/* cara_cross_entropy_ex against a soft target: label smoothing (smoothing = eps in [0, 1): torch's label_smoothing) and the
 * partner's label of a Mixup / CutMix table (mix as in cara_im2col_patches_u8_rows_mix: partner = mix[b][0], t = the fp32 whose
 * bits mix[b][6] holds; mix NULL: t = 0 for every sample) -- timm's mixup_target.  labels are the samples' OWN classes:
 *   ya = labels[b], yb = labels[partner],  q_c = (1 - eps) ((1 - t) [c == ya] + t [c == yb]) + eps / C,
 *   loss[1 + b] = (lse_b - sum_c q_c l_c) / B,  loss[0] = their sum (unscaled),  dlogits = (softmax - q) / B * dscale * loss scale.
 * eps == 0 with t == 0 (with a table or without) gives bit for bit what cara_cross_entropy_ex gives.  ya or yb outside [0, C), a
 * partner outside [0, B) or a t outside [0, 1] (or NaN) is never used as an index: that sample's term, its dlogits row and
 * loss[0] are NaN, the other samples unaffected.  smoothing outside [0, 1): CARA_E_ARG, nothing launched.  found_inf is cleared. */
int cara_cross_entropy_mix(const float* logits, const int64_t* labels, const int* mix, float smoothing, float* loss,
                           float* dlogits, int B, int C, float dscale, const float* loss_scale, float* found_inf, void* stream);
/* cara_cross_entropy_mix with a weight per class and a bias on the logits: class_weight, logit_bias = device fp32 [C], either may
 * be NULL (all ones / all zeros).  With q, ya, yb and t of cara_cross_entropy_mix, all in fp32:
 *   z_c = logits[b][c] + logit_bias[c] (softmax, lse and p are of z),  W_b = sum_c class_weight[c] q_c,
 *   loss[1 + b] = (W_b lse_b - sum_c class_weight[c] q_c z_c) / B,  loss[0] = their sum (unscaled),
 *   dlogits[b][c] = (p_c W_b - class_weight[c] q_c) / B * dscale * loss scale
 * -- torch's cross_entropy(logits + bias, q, weight = class_weight, reduction = "sum") / B.  The divisor is B, not the weight mass
 * of the batch: the loss stays linear in the samples, so dscale and a SUM all-reduce mean what they mean above (weights whose mean
 * over the training samples is 1 keep the loss scale).  The bias enters the loss only (logit-adjusted training): logits is not
 * written.  Both vectors NULL: the launches of cara_cross_entropy_mix, bit for bit.  The guards, the NaNs and the refusals are
 * cara_cross_entropy_mix's; a refused sample reads no class of either vector that its labels name.  The VALUES of the two vectors are
 * not looked at: the caller keeps class_weight finite and >= 0 and logit_bias finite.  found_inf is cleared.                     */
int cara_cross_entropy_bal(const float* logits, const int64_t* labels, const int* mix, float smoothing, const float* class_weight,
                           const float* logit_bias, float* loss, float* dlogits, int B, int C, float dscale,
                           const float* loss_scale, float* found_inf, void* stream);
/* The sigmoid losses on cara_cross_entropy_mix's soft target: binary cross-entropy (timm's BinaryCrossEntropy, torch's
 * binary_cross_entropy_with_logits) and the focal loss (torchvision's sigmoid_focal_loss, extended to a soft target).  The tail
 * arguments from loss on, the labels, mix and smoothing are cara_cross_entropy_mix's.  All in fp32, per element, z = logits[b][c]:
 *   q_c = the soft target there (same ya, yb, t, eps);  target_threshold >= 0:  q_c <- (q_c > target_threshold) ? 1 : 0
 *         (timm's target.gt(thr), decided on the fp32 q_c);  target_threshold < 0: none.
 *   sp(z) = max(z, 0) + log1p(exp(-|z|)),  s+ = sigma(z),  s- = sigma(-z), all from the one exp(-|z|): nothing overflows, and
 *         neither sigmoid is formed as one minus the other.
 *   BCE (gamma == 0 and alpha < 0):  l = pw_c q sp(-z) + (1 - q) sp(z),  dl/dz = s+ (1 - q + pw_c q) - pw_c q, evaluated as
 *         (1 - q) s+ - pw_c q s-;  pw_c = pos_weight[c] (device fp32 [C]) or 1 where pos_weight is NULL.
 *   focal (gamma > 0 or alpha >= 0; pos_weight must be NULL):  ce = q sp(-z) + (1 - q) sp(z),  m = q s- + (1 - q) s+,
 *         a = alpha q + (1 - alpha)(1 - q) (alpha < 0: none, a = 1),  l = a m^gamma ce,
 *         dl/dz = a [(s+ - q) m^gamma + gamma ce m^(gamma - 1) s+ s- (1 - 2 q)].   gamma is 0 or >= 1.
 *   loss[1 + b] = sum_c l / (B D),  D = C (the "mean" of torch and timm) or 1 with sum_classes = 1 (timm's sum_classes);
 *   loss[0] = their sum through the fixed tree (unscaled);  dlogits[b][c] = dl/dz / (B D) * dscale * loss scale.
 * The loss is linear in the samples: dscale, accumulation windows and a SUM all-reduce mean what they mean above.
 * Bit for bit: pos_weight of all ones == pos_weight NULL; dlogits NULL gives the same loss.  The guards and NaNs are
 * cara_cross_entropy_mix's (a refused sample indexes nothing through a label; pos_weight is read by class index only).
 * CARA_E_ARG, nothing launched: smoothing outside [0, 1); target_threshold >= 1 or NaN; gamma negative, in (0, 1) or not finite;
 * alpha > 1 or NaN; pos_weight with a focal parameter; sum_classes outside {0, 1}; NULL logits, labels or loss; B <= 0, C <= 0;
 * dscale not > 0.  The VALUES of pos_weight are not looked at: the caller keeps them finite and >= 0.  found_inf is cleared.   */
int cara_sigmoid_loss(const float* logits, const int64_t* labels, const int* mix, float smoothing, float target_threshold,
                      float gamma, float alpha, const float* pos_weight, int sum_classes, float* loss, float* dlogits,
                      int B, int C, float dscale, const float* loss_scale, float* found_inf, void* stream);
/* Knowledge distillation on cara_cross_entropy_mix's soft target (Hinton et al.; DeiT's hard variant): teacher = device fp32 [B,C],
 * dense, the logits of a teacher for the same samples -- it gets no gradient.  labels, mix, smoothing and the tail arguments from
 * loss on are cara_cross_entropy_mix's, q its soft target, z = logits[b], t = teacher[b], a = alpha in [0, 1], T = temperature.
 * All in fp32, one wave per sample:
 *   soft (hard == 0):  p = softmax(z),  pT = softmax(z / T),  r = softmax(t / T),
 *     loss[1 + b] = [(1 - a)(lse(z) - sum_c q_c z_c) + a T^2 sum_c r_c (log r_c - log pT_c)] / B,
 *     dlogits[b][c] = [(1 - a)(p_c - q_c) + a T (pT_c - r_c)] / B * dscale * loss scale
 *     -- (1 - a) cross_entropy(z, q) + a T^2 kl_div(log_softmax(z / T), softmax(t / T), reduction = "batchmean") and its gradient.
 *     log r_c and log pT_c are x_c (1 / T) - lse(x / T) from ONE function applied to either row, and the sum is taken over their
 *     differences: teacher == logits (the same values) with a == 1 gives a dlogits of exact zeros.
 *   hard (hard == 1):  yt = the lowest class index that attains the maximum of t (cara_eval_accumulate's tie rule),
 *     q' = (1 - a) q + a onehot(yt),  loss[1 + b] = (lse(z) - sum_c q'_c z_c) / B,  dlogits = (p - q') / B * dscale * loss scale;
 *     temperature is not read.
 *   loss[0] = the sum of the terms through the fixed tree (unscaled).  The loss is linear in the samples: dscale, accumulation
 *   windows and a SUM all-reduce mean what they mean above.
 * Bit for bit: alpha == 0 is cara_cross_entropy_mix (the same launches; teacher is not read and may be NULL); dlogits NULL gives the
 * same loss.  The label and mix guards are cara_cross_entropy_mix's.  With alpha > 0 a teacher row that holds a NaN, +inf or -inf
 * makes that sample's term, its dlogits row and loss[0] NaN and is never turned into a class index; every other sample's outputs
 * are the bits they are without it.
 * CARA_E_ARG, nothing launched: alpha outside [0, 1] or NaN; hard outside {0, 1}; with alpha > 0: teacher NULL, and in soft mode a
 * temperature that is not finite, not > 0, or so small that the fp32 1 / temperature is not finite (below about 2.94e-39);
 * everything cara_cross_entropy_mix refuses.  found_inf is cleared.                                                            */
int cara_distill_loss(const float* logits, const float* teacher, const int64_t* labels, const int* mix, float smoothing,
                      float alpha, float temperature, int hard, float* loss, float* dlogits, int B, int C, float dscale,
                      const float* loss_scale, float* found_inf, void* stream);
/* Scoring on the device (test() of vit_cp.py:73-82 without its per-batch host read): for the first n_valid <= B rows of
 * logits fp32 [B,classes] (row stride ldl floats) and labels int64 [B], ADD into `state`, five 64-bit words
 * (cara_eval_state_bytes() = 40 bytes, 8-byte aligned, zeroed by the caller before the first batch):
 *   [0] int64 rows scored   [1] int64 top-1 hits   [2] int64 top-5 hits   [3] double sum of the per-row cross-entropy
 *   [4] int64 rows whose label lies outside [0, classes): such a row raises this word and adds to nothing else.
 * Top-1 ties go to the lowest class index (numpy.argmax); top-5 = the label is among the first five of a stable
 * descending sort (always, with fewer than five classes).  Log-sum-exp in fp32 per row, rows summed in fp64.  Any B,
 * any class count; one launch, a handful of atomicAdd per workgroup (the integer words are exact in any order; the loss
 * word is an fp64 sum whose order is not fixed).                                                                    */
size_t cara_eval_state_bytes(void);
int cara_eval_accumulate(const float* logits, int ldl, const int64_t* labels, int B, int n_valid, int classes,
                         void* state, void* stream);
/* The same launch with an evaluation report: beside `state` (unchanged meaning, the same words) every scored row adds into
 * `report`, device memory of 8-byte words (cara_eval_report_bytes(classes, bins) bytes, 8-byte aligned, zeroed by the
 * caller before the first batch, accumulated across launches):
 *   confusion int64 [classes][classes]  row = label, column = predicted class
 *   bin_count int64 [bins]   bin_hits int64 [bins]   bin_conf double [bins]
 * pred = the lowest class index whose logit equals the row maximum (the top-1 tie rule above: pred == label exactly when
 * the row is a top-1 hit); conf = 1 / sum_c exp(l[c] - max), the top softmax probability, in fp32 from the sum the loss
 * uses; bin = min(bins - 1, (int)(conf * bins)) in fp32.  The row adds 1 to confusion[label][pred] and to bin_count[bin],
 * (pred == label) to bin_hits[bin] and conf to bin_conf[bin] (an fp64 sum whose order is not fixed).  A row whose label
 * lies outside [0, classes) raises word 4 of `state` and touches nothing in `report`.  A row without a finite maximum
 * (a NaN, or no logit above -3e38) is counted in column 0 / bin 0: every index stays inside the buffer.
 * CARA_E_ARG with nothing launched: classes > CARA_EVAL_REPORT_MAX_CLASSES, bins outside [1, CARA_EVAL_REPORT_MAX_BINS],
 * report NULL or not 8-byte aligned, and everything the plain entry refuses.  The byte count is 0 for a refused pair.   */
#define CARA_EVAL_REPORT_MAX_CLASSES 4096
#define CARA_EVAL_REPORT_MAX_BINS 64
size_t cara_eval_report_bytes(int classes, int bins);
int cara_eval_accumulate_report(const float* logits, int ldl, const int64_t* labels, int B, int n_valid, int classes,
                                void* state, void* report, int bins, void* stream);
/* Multi-view evaluation (centre crop + flip, five / ten crops): the V views' logits of every sample -> ONE row per sample, in a
 * form the two entries above score unchanged.  logits fp32 [S*V, classes] (row stride ldl floats), the views of sample s in
 * rows s*V .. s*V+V-1; out fp32 [S, classes] (row stride ldo floats).  All in fp32 with the accurate expf / logf:
 *   CARA_EVAL_COMBINE_PROB   out[s][c] = log((1/V) sum_v softmax(l_{s,v})[c]), formed in the log domain:
 *                            lse_v = m_v + logf(sum_c expf(l_v[c] - m_v)),  a_v = l_v[c] - lse_v,  M = max_v a_v,
 *                            out = M + logf(sum_v expf(a_v - M)) - logf(V), views summed in index order; -inf (not NaN) where M
 *                            is -inf, i.e. the class has probability zero in every view.  The accumulate entries then give
 *                            loss = -log pbar[y], confidence = max pbar, and their rank and tie rules on pbar.
 *   CARA_EVAL_COMBINE_LOGIT  out[s][c] = (sum_v l_{s,v}[c]) / V, summed in view order, the division correctly rounded.
 * V = 1 is legal: log_softmax and a copy.  One launch, one wave per sample; columns >= classes of out are never written.
 * CARA_E_ARG with nothing launched: a NULL pointer, S < 1, V outside [1, CARA_EVAL_MAX_VIEWS], classes < 1, ldl or ldo < classes,
 * an unknown mode, logits or out not 4-byte aligned, out overlapping logits.                                                     */
#define CARA_EVAL_MAX_VIEWS 16
#define CARA_EVAL_COMBINE_PROB 0
#define CARA_EVAL_COMBINE_LOGIT 1
int cara_eval_combine_views(const float* logits, int ldl, int S, int V, int classes, int mode, float* out, int ldo, void* stream);
/* Per-sample predictions: for every batch row b < n_valid of logits fp32 [B,classes] (row stride ldl floats; the rows the two
 * accumulate entries score, cara_eval_combine_views' output included) WRITE row first + b, and only that row, of a device table
 * of n_rows rows: topk_idx int32 [n_rows][k], topk_prob fp32 [n_rows][k] and, with labels int64 [B], loss fp32 [n_rows] and
 * rank int32 [n_rows].  labels NULL: no loss, no rank (both NULL then, and only then).  With l the row, fp32 throughout:
 *   topk_idx[j]   the class at position j of the STABLE DESCENDING sort of the row: ties go to the lowest class index, the rule of
 *                 cara_eval_accumulate.  So topk_idx[0] is the `pred` of cara_eval_accumulate_report, rank == 0 exactly when
 *                 topk_idx[0] == label, and rank < 5 exactly when the label is among the first five slots.  -inf logits (what
 *                 cara_eval_combine_views writes for a class of probability zero) are ordinary values: they sort last, in index
 *                 order.  Slots j >= classes hold index -1 and probability 0.
 *   topk_prob[j]  expf(l[idx_j] - m) / s with m the row maximum and s = sum_c expf(l[c] - m), formed by the same walk over the
 *                 row, in the same order, as the accumulate entries form it (one device function): topk_prob[0] is, bit for bit,
 *                 the `conf` the report bins.  The accurate expf / logf, the division correctly rounded.
 *   loss          (float)((double)(m + logf(s)) - (double)l[label]): the term cara_eval_accumulate adds, rounded once to fp32.
 *   rank          #{c : l[c] > v} + #{c < label : l[c] == v}, v = l[label]: the label's position in that sort.
 * A label outside [0, classes): rank = -1 and loss = NaN; the row's top-k slots are written as for any row.  A row without a
 * finite maximum (the report's case: no logit above -3e38, or only NaN): topk_idx[0] = 0, the other indices -1, all k
 * probabilities and the loss NaN; rank as defined.  A row that holds a NaN beside finite values may give any values.  In every
 * case each index lies in [-1, classes) and nothing outside the row's own slots is written.  Plain stores, no atomics: the same
 * inputs give the same bits, and rows of one table may be filled by launches in any order (and by several processes whose
 * tables are then added as integer words: an unwritten row of a zeroed table adds nothing).
 * One wave per row: the two passes of the accumulate kernel, then k selection rounds over the (cache-resident) row.  Any B, any
 * class count.  CARA_E_ARG with nothing launched: logits, topk_idx or topk_prob NULL; loss / rank not NULL exactly when labels
 * is; k outside [1, CARA_EVAL_PREDICT_MAX_K]; first < 0, n_rows < 0 or first + n_valid > n_rows; logits, topk_idx, topk_prob,
 * loss or rank not 4-byte aligned, labels not 8-byte aligned; B <= 0, n_valid outside [0, B], classes < 1, ldl < classes.   */
#define CARA_EVAL_PREDICT_MAX_K 16
int cara_eval_predict(const float* logits, int ldl, const int64_t* labels /* may be NULL */, int B, int n_valid, int classes,
                      int k, int64_t first, int64_t n_rows,
                      int32_t* topk_idx /* [n_rows][k] */, float* topk_prob /* [n_rows][k] */,
                      float* loss /* [n_rows], NULL iff labels NULL */, int32_t* rank /* [n_rows], NULL iff labels NULL */,
                      void* stream);
/* bf16 <-> fp32 helpers (weight ingest)                                                        */
int cara_f32_to_bf16(const float* src, void* dst, size_t n, void* stream);
int cara_transpose_bf16(const void* src, void* dst, int rows, int cols, void* stream);
/* the same for activation-sized matrices: row strides lds >= cols, ldd >= rows (multiples of 8), 16-byte accesses */
int cara_transpose_bf16_ld(const void* src, long lds, void* dst, long ldd, int rows, int cols, void* stream);

/* ---- CP factor preparation / gradient scatter --------------------- */
/* Geometry of one adapted ViT.  The reference hard-codes dim 768 / heads 12 / depth 12
 * (cara.py:112-125); the same formulas are kept general.                                      */
typedef struct {
  int depth, dim, heads, rank, Rp;
  float scale;                       /* child.s, cara.py:149,159 */
  /* Order of the CP tensorisation of the QKV adapter (image_classification/dim_experiment.py:188-207,264-295).
   * 0 or 4 (src/cara, the default): dW[k,e,h,d] = sum_r R1 A1[3l+k] A2[e] A3[h] A4[d],  A1 [3 depth,R], A2 [dim,R],
   *         A3 [heads,R], A4 [dim/heads,R].
   * 3: dW[k,e,o] = sum_r R1 A1[3l+k] A2[e] A3[o],  A3 [dim,R], no A4.
   * 5: dW[k,e,h,d] = sum_r R1 A1[l] A2[k] A3[e] A4[h] A5[d],  A1 [depth,R], A2 [3,R], A3 [dim,R], A4 [heads,R],
   *    A5 [dim/heads,R].
   * All three are rank-R in (in, out) and run on the same factored kernels; only the factor pack and the
   * gradient scatter differ.
   * 2: dW[k, e * dim + o] = sum_r R1 A1[3l+k] A2[e * dim + o],  A2 [dim * dim, R], no A3 / A4 (NULL): a sum of R DENSE
   *    dim x dim matrices per projection, not low-rank -- the QKV linear then runs in the dense-delta form
   *    (cara_dense_delta_* below; weight_dropout off only) while proj / fc1 / fc2 keep the factored kernels.           */
  int cp_length;
} cara_geom;
/* Pointers to the CP tensors (fp32, shapes of cara.py:112-125 for cp_length 4) or to their gradients.
 * A4 is unused for cp_length 3, A5 only used for cp_length 5 (NULL otherwise).                               */
typedef struct {
  float *A1, *A2, *A3, *A4, *P1, *P2, *P3, *R1, *R2, *bias1, *bias2, *bias3;
  float *A5;
} cara_cp;
/* Per-layer operand pack written by cara_factor_prep (bf16 unless noted), l = 0..depth-1:
 *   Ut_* [Rp,in] (U transposed, K-contiguous), U_* [in,Rp], Vs_* [out,Rp], Vst_* [Rp,out]
 * laid out back to back; offsets via cara_pack_offsets().  Row padding rank..Rp-1 is zero.     */
typedef struct {
  size_t Ut_qkv, U_qkv, Vs_qkv, Vst_qkv;
  size_t Ut_proj, U_proj, Vs_proj, Vst_proj;
  size_t Ut_fc1, U_fc1, Vs_fc1, Vst_fc1;
  size_t Ut_fc2, U_fc2, Vs_fc2, Vst_fc2;
  size_t bias_proj, bias_fc1, bias_fc2;      /* fp32: b + s*CP_bias (needs backbone bias)      */
  size_t layer_stride;                       /* bytes between consecutive layers               */
  size_t total;                              /* bytes for all layers                           */
} cara_pack_layout;
int cara_pack_offsets(const cara_geom* g, cara_pack_layout* out);            /* host only */
/* Build every layer's operand pack from the CP tensors in one launch.  base_bias_* are the
 * frozen fp32 biases of proj/fc1/fc2, [depth, out] contiguous.                                 */
int cara_factor_prep(const cara_geom* g, const cara_cp* cp, const float* base_bias_proj,
                     const float* base_bias_fc1, const float* base_bias_fc2, void* pack,
                     void* stream);
/* Scatter per-layer skinny gradients onto the 12 shared tensors (A.4).  dU_x / dVs_x are fp32
 * [depth, in|out, Rp]; dc_x fp32 [depth, out] (column sums of dY of proj/fc1/fc2).  grads are
 * OVERWRITTEN.  scratch: cara_factor_grad_scratch_bytes(g) bytes (partials, summed in a fixed
 * order: bitwise reproducible).                                                                */
typedef struct {
  const float *dU_qkv, *dVs_qkv, *dU_proj, *dVs_proj, *dU_fc1, *dVs_fc1, *dU_fc2, *dVs_fc2;
  const float *dc_proj, *dc_fc1, *dc_fc2;
} cara_layer_grads;
size_t cara_factor_grad_scratch_bytes(const cara_geom* g);
int cara_factor_grad_reduce(const cara_geom* g, const cara_cp* cp, const cara_layer_grads* lg,
                            const cara_cp* grads, void* scratch, void* stream);
/* The same under a loss scale: every gradient written is multiplied by 1 / *loss_scale (device float; NULL = 1), and
 * *found_inf (device float; NULL = no check) is set to 1 when a written value is not finite.                          */
int cara_factor_grad_reduce_ex(const cara_geom* g, const cara_cp* cp, const cara_layer_grads* lg,
                               const cara_cp* grads, void* scratch, const float* loss_scale, float* found_inf,
                               void* stream);

/* ---- order-2 QKV tensorisation (image_classification/dim_experiment.py:203-207,293-297; cara_geom::cp_length == 2) ---- */
/* Dm bf16 [depth][3 dim, dim] with Dm[l][k dim + o][e] = s * sum_r R1[r] A1[3l+k, r] A2[e dim + o, r] (the second B operand,
 * cara_gemm_args::B3, of the QKV linear next to the frozen weight) and Dmt bf16 [depth][dim, 3 dim] its transpose (for dX). */
int cara_dense_delta_materialize(const cara_geom* g, const cara_cp* cp, void* Dm, void* Dmt, void* stream);
/* From dD fp32 [depth][3][dim (e), dim (o)] = x^T dY_k per block and projection (cara_gemm_tn_f32 + cara_sum_slabs_f32) to the
 * gradients of CP_A1, CP_A2, CP_R1 (OVERWRITTEN in `grads`; run it AFTER cara_factor_grad_reduce, which for this order leaves
 * CP_A1 / CP_A2 alone and writes a zero CP_R1).  Fixed summation order.  scratch: cara_dense_delta_grad_scratch_bytes(g). */
size_t cara_dense_delta_grad_scratch_bytes(const cara_geom* g);
int cara_dense_delta_grad(const cara_geom* g, const cara_cp* cp, const float* dD, const cara_cp* grads, void* scratch, void* stream);
/* out[j] = sum_z slabs[z * slab_stride + j], j < count (fixed order): the split-K slabs of cara_gemm_tn_f32 into one matrix */
int cara_sum_slabs_f32(const float* slabs, int nslab, size_t slab_stride, size_t count, float* out, void* stream);

/* ---- optimiser step (image_classification/vit_cp.py:185 `torch.optim.AdamW(trainable, ...)`, :50 `opt.step()`) ---- */
/* torch.optim.AdamW's arithmetic (amsgrad off, maximize off) over up to 32 fp32 tensors in ONE launch:
 *   p *= 1 - lr wd;  m += (1 - beta1)(g - m);  v = beta2 v + (1 - beta2) g g;
 *   p -= lr / bias_correction1 * m / (sqrt(v) / bias_correction2_sqrt + eps)
 * with bias_correction1 = 1 - beta1^step and bias_correction2_sqrt = sqrt(1 - beta2^step) computed by the caller (in double, as
 * torch does on the host).  `group` picks the tensor's lr / weight_decay (param groups; betas and eps are shared).
 * The struct travels by value into the kernel: nothing lives in device memory, a changed lr costs nothing.          */
#define CARA_ADAMW_MAX_TENSORS 32
#define CARA_ADAMW_MAX_GROUPS 4
typedef struct {
  float* p; const float* g; float* m; float* v;   /* parameter, gradient, exp_avg, exp_avg_sq: n fp32 each */
  size_t n;
  int group;
} cara_adamw_tensor;
typedef struct {
  cara_adamw_tensor t[CARA_ADAMW_MAX_TENSORS];
  int ntensors;
  int step;                                        /* 1-based step count (validation only; the corrections come below) */
  float lr[CARA_ADAMW_MAX_GROUPS], weight_decay[CARA_ADAMW_MAX_GROUPS];
  float one_minus_beta1, beta2, one_minus_beta2, eps;
  float bias_correction1, bias_correction2_sqrt;
  /* device float or NULL: when *skip_flag != 0 the launch changes nothing (a step whose gradients overflowed under the
   * loss scale of the IEEE-half build: cara_vit_shape::found_inf, all-reduced with the gradients)                     */
  const float* skip_flag;
  /* device float[1 + CARA_ADAMW_MAX_GROUPS] or NULL: { step count t, lr of group 0, 1, ... }.  When given, the kernel takes the
   * learning rates from it and computes both bias corrections from t itself (`step`, `lr`, `bias_correction*` above are ignored):
   * nothing that changes from step to step travels in the launch arguments, so a launch captured into a hipGraph stays correct
   * under replay -- the host rewrites the five floats (stream-ordered) before each replay.                                     */
  const float* dyn;
} cara_adamw_args;
int cara_adamw_step(const cara_adamw_args* a, void* stream);
/* Dynamic loss scale of the IEEE-half operand build, entirely on the device (no host synchronisation anywhere in a step).
 * state (device float[4]) = { scale, clean steps since the last change, steps skipped so far, unused }.  Once per step,
 * AFTER the all-reduce and BEFORE the optimiser: *found_inf != 0 (some rank wrote a non-finite gradient) -> scale *= backoff,
 * counter = 0, skipped += 1; otherwise counter += 1 and, at `interval` clean steps, scale *= growth (capped at max_scale),
 * counter = 0.  torch.amp.GradScaler's rule.  found_inf is left as it is (cara_adamw_args::skip_flag reads it next).    */
int cara_amp_update(float* state, const float* found_inf, float growth, float backoff, int interval, float max_scale,
                    void* stream);
/* Gradient accumulation over one flat fp32 buffer: dst[i] = a[i] + b[i], i < n, one fp32 rounding each; b == NULL copies a.
 * dst may be a or b (an element is read and written by the same thread).  Any n >= 1 and any 4-byte-aligned pointers: 16-byte
 * accesses where the three pointers share one residue mod 16, dword accesses otherwise.  The engine's flat buffer carries the
 * found-inf word as its last element; adding it along keeps "some micro-step overflowed" non-zero.  Only enqueues.          */
int cara_grad_accumulate(float* dst, const float* a, const float* b, size_t n, void* stream);
/* torch.nn.utils.clip_grad_norm_(norm_type = 2) over one flat fp32 buffer g[n], 1 <= n <= 2^31, in two launches without atomics:
 * launch 1 writes one partial sum of squares per chunk of 8192 elements into scratch (cara_grad_clip_scratch_bytes(n) bytes;
 * 0 for an n outside the range); in launch 2 EVERY workgroup adds all partials in the same fixed order (the tree is stated in
 * cara_amd/csrc/optim.hip), so each holds the identical total, forms norm = sqrtf(total) and coef = min(1, max_norm /
 * (norm + 1e-6f)) and multiplies its own chunks by coef; workgroup 0 writes out[0] = norm, out[1] = coef (device float[2]).
 * Bitwise reproducible run to run, and equal on all ranks that hold equal buffers.  coef == 1: g is not written at all.
 * found_inf (device float or NULL) != 0: g is left untouched and out[1] = 1 -- the step is skipped anyway (cara_amp_update,
 * cara_adamw_args::skip_flag) and Inf x 0 must not put NaNs into the gradients.  A NaN norm gives a NaN coef (torch.clamp's rule).
 * max_norm > 0; +inf only measures.  Both launches only enqueue on `stream` and capture into a hipGraph.               */
size_t cara_grad_clip_scratch_bytes(size_t n);
int cara_grad_clip(float* g, size_t n, float max_norm, float* scratch, const float* found_inf, float* out, void* stream);
/* Exponential moving average of up to CARA_ADAMW_MAX_TENSORS fp32 tensors in ONE launch: ema[i][j] moves towards param[i][j] by
 * weight = 1 - decay, j < n[i].  ema, param and n are HOST arrays of ntensors entries (1 <= ntensors <= CARA_ADAMW_MAX_TENSORS), read
 * during the call and carried by value in the kernel arguments: no table in device memory.  weight_dev == NULL: the by-value weight is
 * used; otherwise the kernel reads that device float (a launch captured into a hipGraph then follows a decay that warms up).
 * Per element, in fp32, every operation a single IEEE operation (no fma) -- torch.lerp's definition:
 *   w <  0.5:  e = e + w * (p - e)
 *   otherwise: e = p - (p - e) * (1 - w)
 * so p == e gives e back and w == 1 gives p, bitwise (-0 at w < 0.5 comes back as +0).  16-byte accesses for a tensor whose two
 * pointers are both 16-byte aligned, dword accesses otherwise: the same bits.  param is never written.
 * CARA_E_ARG, nothing launched: a null array or entry, n[i] == 0, a pointer that is not 4-byte aligned, ema[i] == param[i], ntensors
 * out of range, weight_dev == NULL with !(0 <= weight <= 1) (a NaN too).  A device weight outside [0, 1] or NaN: the kernel
 * writes nothing.  Only enqueues.                                                                                              */
int cara_ema_update(int ntensors, float* const* ema, const float* const* param, const size_t* n, float weight,
                    const float* weight_dev, void* stream);
/* Sharpness-aware minimisation (Foret et al.) around the second pass of a step, cara_ema_update's scheme: param, grad, backup and n
 * are HOST arrays of ntensors entries (1 <= ntensors <= CARA_ADAMW_MAX_TENSORS), carried by value in the kernel arguments; ONE launch
 * each; 16-byte accesses for a tensor whose pointers are all 16-byte aligned, dword accesses otherwise: the same bits.
 * cara_sam_perturb: backup[i][j] = param[i][j] (bitwise) for every element, then, with norm a device float holding the global L2 norm
 * of all grad tensors (out[0] of a measuring cara_grad_clip),
 *   scale = rho / (norm + 1e-12f)          two IEEE fp32 operations, the same in every thread (1e-12: the published implementation's)
 *   param = param + scale * grad           one fp32 multiply, then one fp32 add -- no fma
 * found_inf (device float or NULL) != 0, or a norm that is not finite: the backup is written all the same and param is left untouched.
 * Workgroup 0 writes state (device float[4]) = { carry, norm read, scale applied, 0 }: carry = *found_inf (0 for NULL), and the scale
 * applied is 0 where param was left untouched.  grad is never written.
 * cara_sam_restore: param[i][j] = backup[i][j], a copy of the bits (-0, subnormals and NaN payloads come back: never param - e), and,
 * where found_inf is given, one thread does *found_inf += state[0] -- the cross-entropy launch of the second pass has cleared the
 * word, and an overflow of the first pass must still skip the step and back the loss scale off, once.
 * CARA_E_ARG, nothing launched: a null array or entry, n[i] == 0, ntensors out of range, a pointer that is not 4-byte aligned,
 * backup[i] overlapping param[i] or grad[i], rho < 0 or not finite, a null norm or state.  Both only enqueue and capture into a
 * hipGraph.                                                                                                                        */
int cara_sam_perturb(int ntensors, float* const* param, const float* const* grad, float* const* backup, const size_t* n, float rho,
                     const float* norm, const float* found_inf, float* state, void* stream);
int cara_sam_restore(int ntensors, float* const* param, const float* const* backup, const size_t* n, const float* state,
                     float* found_inf, void* stream);

/* ---- exact weight-space dropout mode (the reference's train-mode arithmetic, cara.py:35,57,81,92) ---- */
/* keep(o,i) of linear `linear_id` = (cara_weight_dropout_hash(o*in + i, seed, linear_id) >> 8) >= p * 2^24
 * (host-callable mirror of the device hash, so that tests and the oracle can rebuild the masks).             */
unsigned cara_weight_dropout_hash(unsigned idx, unsigned seed, unsigned linear_id);
/* Weff bf16 [out,in] = W + keep/(1-p) * (Vs U^T): W bf16 [out,in], U bf16 [in,Rp], Vs bf16 [out,Rp] (= s g (.) V,
 * the operand pack of cara_factor_prep).  p = 0 is the eval-time merge of the reference's dW into W.
 * W == NULL: only the masked delta keep/(1-p) * (Vs U^T) is written -- the B3 operand of cara_gemm_args, which keeps
 * an adapter far below W's bf16 ulp (zero-initialised factors early in training) from being rounded away.        */
int cara_materialize_merge(const void* W, const void* U, const void* Vs, int Rp, int out, int in, float p,
                           unsigned seed, unsigned linear_id, void* Weff, void* stream);
/* From the dense weight gradient dW (= dY^T X, given as `nslab` split-K partial slabs of fp32 [out,in], slab_stride
 * floats apart, summed on the fly) to the skinny quantities cara_factor_grad_reduce takes:
 * dVs[o,r] = sum_i keep/(1-p) dW[o,i] U[i,r], dU[i,r] = sum_o keep/(1-p) dW[o,i] Vs[o,r] (fp32 [out,Rp] / [in,Rp],
 * overwritten, fixed summation order; ONE pass over dW for both).  scratch: cara_dropout_grad_scratch_bytes(out, in, Rp).
 * dW needs only the alignment of a float and slab_stride may be any number of floats: the entry point reads dW sixteen bytes at
 * a time where in % 4 == 0, dW is 16-byte aligned and (nslab == 1 or slab_stride % 4 == 0), and element by element otherwise --
 * the same sums in the same order, the same bits.  U and Vs are rows of Rp 16-bit values, 16-byte aligned (the operand pack's). */
size_t cara_dropout_grad_scratch_bytes(int out, int in, int Rp);
int cara_dropout_grad_contract(const float* dW, int nslab, size_t slab_stride, const void* U, const void* Vs, int Rp,
                               int out, int in, float p, unsigned seed, unsigned linear_id, float* dU, float* dVs,
                               void* scratch, void* stream);
/* out fp32 [N] = column sums of a bf16 [M, ld] matrix (dc = sum_m dY), fixed order; scratch:
 * cara_colsum_scratch_bytes(N).  X needs only the alignment of its elements and ld >= N: rows are read sixteen bytes at a time
 * where ld % 8 == 0 and X is 16-byte aligned, element by element otherwise (the same order, the same bits).       */
size_t cara_colsum_scratch_bytes(int N);
int cara_colsum_bf16(const void* X, int ld, int M, int N, float* out, void* scratch, void* stream);

/* ---- whole adapted ViT: forward and backward as stream-ordered kernel sequences ------------ */
/* What model(x) / loss.backward() of vit_cp.py:46-49 run, for the factored adapters.  Both calls
 * only enqueue kernels on `stream` (no allocation, no sync): capturable in a hipGraph.         */
typedef struct {           /* frozen backbone (timm 0.4.12 VisionTransformer), device pointers  */
  const void* patch_w;     /* bf16 [dim, chans*patch*patch]   (patch_embed.proj.weight)         */
  const float* patch_b;    /* fp32 [dim]                                                        */
  const float* cls;        /* fp32 [dim]                      (cls_token)                       */
  const float* pos;        /* fp32 [tokens, dim]              (pos_embed)                       */
  const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;   /* fp32 [depth, dim]                            */
  const void *qkv_w, *qkv_wt;   const float* qkv_b;    /* bf16 [depth,3dim,dim], [depth,dim,3dim] */
  const void *proj_w, *proj_wt; const float* proj_b;   /* bf16 [depth,dim,dim] both              */
  const void *fc1_w, *fc1_wt;   const float* fc1_b;    /* bf16 [depth,4dim,dim], [depth,dim,4dim] */
  const void *fc2_w, *fc2_wt;   const float* fc2_b;    /* bf16 [depth,dim,4dim], [depth,4dim,dim] */
  const float *norm_g, *norm_b; /* fp32 [dim]                                                    */
  /* optional (NULL = unused): the eight matrices above once more as K-panel-major images, per layer
   * [K/32][N][32] with N x K the shape of the row-major matrix (cara_pack_b_panels, cara_gemm_args::Bp) */
  const void *qkv_wp, *qkv_wtp, *proj_wp, *proj_wtp, *fc1_wp, *fc1_wtp, *fc2_wp, *fc2_wtp;
} cara_vit_weights;
typedef struct {
  int B, img, patch, chans, tokens, num_classes;
  float eps;
  /* weight-space dropout on the materialised adapters (cara.py:35,57,81,92).  0 = off: the factored path
   * (eval semantics, and the fast training default: the mask does not factor).  1 = exact: every
   * linear runs on W_eff = W + keep/(1-p) dW (cara_materialize_merge, linear id 4*layer + {qkv,proj,fc1,fc2},
   * seed `wd_seed`, which the caller changes every step) and the adapter gradients come from the dense
   * dW = dY^T X.  The workspace is larger in this mode (cara_vit_workspace_bytes sees the flag).           */
  int wd_exact;
  float wd_p;
  unsigned wd_seed;
  /* 1: no backward will follow this forward (eval / no_grad).  The forward then skips what only the backward
   * reads -- the bf16 pre-activation of fc1 (77 MB per block at bs 64), T^T of the adapter products -- and
   * cara_vit_backward on that workspace is an error until a forward with inference = 0 has run.
   * cara_vit_workspace_bytes sees the flag too (without wd_exact): two activation sets, which the blocks take in turn,
   * and none of the backward's regions -- a prefix of the training layout, so a forward with inference = 1 runs on a
   * workspace of either size with the same launches and the same logits, bit for bit.  cara_vit_backward with
   * inference = 1 returns CARA_E_ARG.                                                                       */
  int inference;
  /* Loss scaling (the IEEE-half operand build; both NULL otherwise).  cara_vit_backward is linear in dlogits: a caller that
   * scaled dlogits by S = *loss_scale (device float) gets every gradient it writes multiplied by 1/S here, in the kernels
   * that write them (no separate unscale launch), and *found_inf (device float, zeroed by the caller or by
   * cara_cross_entropy_ex) is set to 1 when a written gradient is not finite.                                           */
  const float* loss_scale;
  float* found_inf;
  /* The readout.  0: the final LayerNorm on the cls row, then the head (timm's global_pool = "token").  1: the mean of the patch
   * tokens (rows 1 .. tokens - 1 of the last block's output, no LayerNorm in front), then LayerNorm with cara_vit_weights::norm_g /
   * norm_b -- which carry fc_norm's parameters in this mode -- then the head (global_pool = "avg" with fc_norm).  The last block then
   * runs on all its rows, the workspace holds two more fp32 [B,dim] rows (cara_vit_workspace_bytes sees the field; with 0 every size
   * is what it was), and the backward spreads the pooled gradient over the patch rows.  Not with wd_exact; any other value:
   * CARA_E_ARG.                                                                                                                */
  int pool;
} cara_vit_shape;
size_t cara_vit_workspace_bytes(const cara_geom* g, const cara_vit_shape* s);
/* Both calls are stateless (everything lives in the caller's workspace and runs in order on the caller's stream):
 * any number of workspaces / streams / host threads may be in flight at once, one workspace per concurrent call.
 * images fp32 [B,chans,img,img]; droppath fp32 [depth,2,B] per-sample branch multipliers
 * (mask/keep_prob of timm DropPath) or NULL; head_w fp32 [classes,dim], head_b fp32 [classes];
 * logits fp32 [B,classes].  The workspace must be zero-filled once before its first use and
 * must not be touched between a forward and its backward.                                      */
int cara_vit_forward(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w,
                     const cara_cp* cp, const float* head_w, const float* head_b, const float* images,
                     const float* droppath, void* workspace, float* logits, void* stream);
/* cara_vit_forward with the image given as uint8 pixels [B,chans,img,img] and the per-channel mean / std (device fp32
 * [chans]) of the reference's Normalize: the patch rows come from cara_im2col_patches_u8, every later stage is shared.  */
int cara_vit_forward_u8(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w,
                        const cara_cp* cp, const float* head_w, const float* head_b, const unsigned char* pixels,
                        const float* mean, const float* std, const float* droppath, void* workspace, float* logits,
                        void* stream);
/* cara_vit_forward_u8 on B images of a whole resident split (pixels uint8 [n_split,chans,img,img]) chosen by the device
 * index vector rows (int64 [B]): the patch rows come from cara_im2col_patches_u8_rows (bad: its counter, may be NULL), every
 * later stage is shared; on a workspace of either size, and a cara_vit_backward may follow as after cara_vit_forward.      */
int cara_vit_forward_u8_rows(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w,
                             const cara_cp* cp, const float* head_w, const float* head_b, const unsigned char* pixels,
                             int n_split, const int64_t* rows, const float* mean, const float* std, const float* droppath,
                             void* workspace, float* logits, int* bad, void* stream);
/* cara_vit_forward_u8_rows on a split of Hs x Ws pixels (pixels uint8 [n_split,chans,Hs,Ws], any size) read through a crop
 * box per sample (boxes device int32 [B,5]): the patch rows come from cara_im2col_patches_u8_rows_crop, every later stage is
 * shared, the workspace is that of cara_vit_workspace_bytes unchanged, and a cara_vit_backward may follow.                 */
int cara_vit_forward_u8_rows_crop(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w,
                                  const cara_cp* cp, const float* head_w, const float* head_b, const unsigned char* pixels,
                                  int n_split, int Hs, int Ws, const int64_t* rows, const int* boxes, const float* mean,
                                  const float* std, const float* droppath, void* workspace, float* logits, int* bad,
                                  void* stream);
/* cara_vit_forward_u8_rows_crop with a Mixup / CutMix table (mix device int32 [B,8], cara_im2col_patches_u8_rows_mix; boxes may
 * be NULL on a split of the model's size): only the patch rows differ; workspace and backward unchanged.                    */
int cara_vit_forward_u8_rows_mix(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w,
                                 const cara_cp* cp, const float* head_w, const float* head_b, const unsigned char* pixels,
                                 int n_split, int Hs, int Ws, const int64_t* rows, const int* boxes, const int* mix,
                                 const float* mean, const float* std, const float* droppath, void* workspace, float* logits,
                                 int* bad, void* stream);
/* cara_vit_forward_u8_rows_mix with a colour-jitter / erase table (aug device int32 [B,16] and stat_scratch of
 * cara_aug_stat_bytes(B) bytes, cara_im2col_patches_u8_rows_aug; mix and boxes may each be NULL): only the patch rows differ;
 * workspace and backward unchanged.                                                                                          */
int cara_vit_forward_u8_rows_aug(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w,
                                 const cara_cp* cp, const float* head_w, const float* head_b, const unsigned char* pixels,
                                 int n_split, int Hs, int Ws, const int64_t* rows, const int* boxes, const int* mix,
                                 const int* aug, void* stat_scratch, const float* mean, const float* std, const float* droppath,
                                 void* workspace, float* logits, int* bad, void* stream);
/* Patch dropout: the forward on a kept subset of the patch tokens.  cara_vit_shape::tokens may be anything in [2, (img/patch)^2 + 1]
 * for cara_vit_workspace_bytes, cara_vit_backward and the two entries below; every per-token region is sized by it, and at tokens ==
 * (img/patch)^2 + 1 every size is what it was.  The entries above take tokens == (img/patch)^2 + 1 only (CARA_E_ARG otherwise, nothing
 * launched: they write all patch rows).  keep device int32 [B,K] with K == tokens - 1 (CARA_E_ARG otherwise), bad may be NULL:
 * the patch rows come from cara_im2col_patches_keep / cara_im2col_patches_u8_rows_keep (boxes, mix, aug each NULL or not; stat_scratch
 * with aug), the tokens from cara_assemble_tokens_keep; the blocks, the final norm and the head see 1 + K tokens and know nothing of
 * the subset -- the launches of a model whose grid has K patches, on a workspace of cara_vit_workspace_bytes for this shape; a
 * cara_vit_backward with the same shape may follow (the patch embedding and pos are frozen: the backward reaches nothing in front of
 * the blocks).  With keep[b][j] = j, K = (img/patch)^2, logits and every gradient are bit for bit those of the entry without keep.    */
int cara_vit_forward_keep(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w, const cara_cp* cp,
                          const float* head_w, const float* head_b, const float* images, const int* keep, const float* droppath,
                          void* workspace, float* logits, int* bad, void* stream);
int cara_vit_forward_u8_rows_keep(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w, const cara_cp* cp,
                                  const float* head_w, const float* head_b, const unsigned char* pixels, int n_split, int Hs, int Ws,
                                  const int64_t* rows, const int* boxes, const int* mix, const int* aug, void* stat_scratch,
                                  const int* keep, const float* mean, const float* std, const float* droppath, void* workspace,
                                  float* logits, int* bad, void* stream);
/* cara_vit_forward_u8_rows_keep with the patch rows of cara_im2col_patches_u8_rows_ra: ra and ra_scratch (cara_ra_stat_bytes(B)
 * bytes) are required, boxes / mix / aug / keep each NULL or not; without keep, tokens == (img/patch)^2 + 1.                       */
int cara_vit_forward_u8_rows_ra(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w, const cara_cp* cp,
                                const float* head_w, const float* head_b, const unsigned char* pixels, int n_split, int Hs, int Ws,
                                const int64_t* rows, const int* boxes, const int* mix, const int* aug, void* stat_scratch,
                                const int* ra, void* ra_scratch, const int* keep, const float* mean, const float* std,
                                const float* droppath, void* workspace, float* logits, int* bad, void* stream);
/* dlogits fp32 [B,classes] -> grads of the 12 CP tensors (overwritten), dhead_w, dhead_b.       */
int cara_vit_backward(const cara_geom* g, const cara_vit_shape* s, const cara_vit_weights* w,
                      const cara_cp* cp, const float* head_w, const float* dlogits, const float* droppath,
                      void* workspace, const cara_cp* grads, float* dhead_w, float* dhead_b, void* stream);
/* classifier head backward on its own (used by the two above):
 * dW[c,d] = sum_b dl[b,c] xn[b,d]; db[c] = sum_b dl[b,c]; dxn bf16 [B,D] = dl W               */
int cara_head_backward(const float* dlogits, const void* xn_bf16, const float* head_w, float* dhead_w,
                       float* dhead_b, void* dxn_bf16, int B, int classes, int D, void* stream);
/* final LayerNorm of the B cls rows (row stride ldx floats) + classifier head, in fp32 throughout:
 * logits fp32 [B,classes] = LN(x) head_w^T + head_b; also writes LN(x) as 16-bit xn [B,D] and mean / rstd [B]
 * (what cara_head_backward and the final LayerNorm's backward read).  The head is 0.1 % of the work; rounding its two
 * operands to 16 bits was 2.8e-4 (fp16) / 2.4e-3 (bf16) of logit error for nothing (tools/fp16_sim_study.py).        */
int cara_head_forward(const float* x, long ldx, const float* gamma, const float* beta, const float* head_w,
                      const float* head_b, void* xn_16, float* mean, float* rstd, float* logits, int B, int classes,
                      int D, float eps, void* stream);
/* The mean-pooled readout (timm's global_pool = "avg" behind fc_norm; cara_vit_shape::pool = 1), both HBM-bound, no atomics:
 * the same input gives the same bits on every run.  x fp32 [B,tokens,D], out fp32 [B,D]:
 *   out[b,:] = mean over t in [first, tokens) of x[b,t,:]
 * in fp32, in a fixed order; rows below `first` (the cls token: first = 1) are never read, and with one token the row goes
 * through bit for bit.  CARA_E_ARG, nothing launched: a NULL pointer, B <= 0, first < 0, tokens <= first, D <= 0, D % 4 != 0.  */
int cara_token_mean(const float* x, int B, int tokens, int first, int D, float* out, void* stream);
/* Its backward, into the residual-stream gradient of the last block and the dY of that block's fc2:
 *   dx fp32 [B,tokens,D]: dx[b,t,:] = dpool[b,:] / (tokens - first) for t >= first, exactly 0 below;
 *   dyb bf16: the 16-bit values of rowscale[b] * dx (rowscale fp32 [B], NULL = 1), row-major [B*tokens, D], or K-panel-major
 *   [D/32][dyb_panels][32] when dyb_panels > 0 (>= B*tokens rows per panel, D % 32 == 0): cara_layernorm_bwd_ex's layout rule.
 * Every element of both outputs is written (no memset in front).  dpool stays in whatever scale it has: nothing is unscaled or
 * tested for inf here.  Refusals as above.                                                                                    */
int cara_token_mean_bwd(const float* dpool, const float* rowscale, int B, int tokens, int first, int D, float* dx, void* dyb,
                        int dyb_panels, void* stream);

/* ---- ABI self-description ------------------------------------------------------------------- */
/* sizeof() of the structs above as THIS library was compiled, so that a binding can assert that its own mirror of a
 * struct (ctypes.Structure, cgo, JNA ...) has the same size before it hands one over: a field missing at the end of
 * the mirror would otherwise make the library read past it.  cara_sizeof_struct(CARA_STRUCT_*) returns 0 for an
 * unknown id.                                                                                                   */
enum {
  CARA_STRUCT_GEMM_ARGS = 0, CARA_STRUCT_GEOM, CARA_STRUCT_CP, CARA_STRUCT_PACK_LAYOUT, CARA_STRUCT_LAYER_GRADS,
  CARA_STRUCT_VIT_WEIGHTS, CARA_STRUCT_VIT_SHAPE, CARA_STRUCT_TS_REDUCE, CARA_STRUCT_LINEAR, CARA_STRUCT_ADAMW_ARGS,
  CARA_STRUCT_COUNT
};
size_t cara_sizeof_struct(int which);
size_t cara_sizeof_gemm_args(void);      /* == cara_sizeof_struct(CARA_STRUCT_GEMM_ARGS) */

/* ---- the step's one collective (optional) ------------------------------------------------------ */
/* SUM all-reduce, in place, of `count` fp32 values on `stream` through RCCL: the flat gradient buffer of a data-parallel
 * step (the reference: DistributedDataParallel's bucketed all-reduce, image_classification/vit_cp.py's launcher; here ONE
 * call per step -- the buffer is 121 923 gradients + the found-inf word at the headline configuration, pre-scaled by
 * 1 / world size at the cross-entropy, cara_cross_entropy_ex).  nccl_comm = the caller's ncclComm_t.  librccl is looked up at
 * the first call: CARA_E_LAUNCH when the process has none.  The Python side of this repository uses torch.distributed
 * (backend "nccl" = RCCL), whose communicator is not exposed; a C++ host that owns one calls this.                      */
int cara_allreduce_flat(void* nccl_comm, float* buf, size_t count, void* stream);

/* ---- diagnostics ---------------------------------------------------------------------------- */
/* HIP-event brackets around the kernels of chosen call sites INSIDE cara_vit_forward / cara_vit_backward, recorded
 * on the compute stream, so that a benchmark can read per-kernel launch durations from within its timed region
 * (bench.py: `roofline`).  mask = bit set of CARA_SITE_* (0 = off); only the full-size blocks l with l % every == every / 2
 * are bracketed (every = 1: all of them; never block 0 otherwise -- its qkv dX and LayerNorm-1 backward do not exist).  Every bracket idles the chip for ~15 us (three event records), so a timed run brackets one site
 * on a few layers per step.  Read after synchronising: avg_ms = mean duration of the last (up to CARA_SITE_RING)
 * brackets of that site minus marker_ms, the mean of the EMPTY bracket recorded behind each (the markers' own
 * cost); launches = brackets recorded since cara_profile_sites() (0: the site never ran).  A GEMM site holds exactly the GEMM launch (with the
 * transposed skinny products that ride in it), a SKINNY site the separate cara_skinny_xu passes.
 * This is the ONLY process-global state of the library: diagnostic, off by default, not thread-safe.            */
enum {
  CARA_SITE_QKV_FWD = 0, CARA_SITE_PROJ_FWD, CARA_SITE_FC1_FWD, CARA_SITE_FC2_FWD,
  CARA_SITE_QKV_BWD, CARA_SITE_PROJ_BWD, CARA_SITE_FC1_BWD, CARA_SITE_FC2_BWD,
  CARA_SITE_ATTN_FWD, CARA_SITE_ATTN_BWD,
  CARA_SITE_LN1_FWD, CARA_SITE_LN2_FWD, CARA_SITE_LN1_BWD, CARA_SITE_LN2_BWD,
  CARA_SITE_SKINNY_FWD, CARA_SITE_SKINNY_BWD,
  CARA_SITE_COUNT
};
#define CARA_SITE_RING 64
int cara_profile_sites(unsigned long long mask, int every);
int cara_profile_site_read(int site, float* avg_ms, float* marker_ms, int* launches);   /* host pointers */
/* One ds_read_b64_tr_b16 per lane (64 lanes) over an LDS image of 16-bit values sm[i] = i, lane l
 * reading at byte address byte_addr[l] (device int[64], multiples of 8, < 16384); out = device
 * short[256] (4 per lane).  Pins the lane semantics the attention kernels rely on.             */
int cara_debug_tr_probe(const int* byte_addr, short* out, void* stream);
/* The attention kernels' transposed fragment of a staged [N,64] bf16 matrix: out bf16 [64 lanes][8]. */
int cara_debug_tr_frag(const void* src, void* out, int N, int cbase, int base, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CARA_HIP_H */
