// The MT x 256 x 64 one-workgroup-per-CU GEMM tile (gemm8.hip) as seen by the front end in gemm.hip (gemm_plan).
#pragma once
#include "common.h"

// one transposed skinny product riding in the launch (the fields of TsProblem, tskinny_body.h)
struct cara_g8_product {
  const void* X; const void* Gt;
  float* slabs; float* cs_slabs;
  int ldx, K1, nchunks, nblk;
};
struct cara_g8_riders {
  cara_g8_product a, b;
  int ldg, M, any_cs, nt;
};

// what the tile does with a product it takes (filled by cara_gemm8_plan)
struct cara_g8_plan {
  int mt;               // rows per tile: 160, or 256 (the yardstick form: plain products)
  int mode;             // 0 plain product; 1 K-extension with T given; 2 the adapter inside, T by the tile waves; 3 T by helper waves
  bool helpers;         // helper waves stream the riders / compute T: the riding products write one slab per WAVE
  bool dv;              // dVs (+ dc) of the GEMM's own linear out of its A sub-buffers (cara_gemm_args::er_Tt with CARA_EPI_BF16)
  int tiles_n, nwg;     // column tiles, tile workgroups (riding products as workgroups sit behind them)
  int block, lds;       // threads per workgroup, dynamic LDS bytes
  int stagger;          // CARA_GEMM8_STAGGER for the plain products of several rounds, else 0
};
// Does the tile of mt rows take the product, and how?  0 = no (the caller runs the 128 x 128 x 32 family); 1 = yes, riding products
// (riders_nt = their column tiles of 16, 0 = none; riders_colsum: the second one leaves column sums) as workgroups behind the tiles:
// one slab per tskinny BLOCK; 2 = yes, with helper waves.  Host arithmetic on the arguments only.  *out (may be NULL) is filled on
// 1 / 2, and cara_gemm8_launch launches exactly that: a yes is never taken back.
int cara_gemm8_plan(const cara_gemm_args* a, int mt, int riders_nt, int riders_colsum, cara_g8_plan* out);
// CARA_OK, or CARA_E_LAUNCH on a failed launch.  ts: the pair of riding products the plan was made for, or NULL.
int cara_gemm8_launch(const cara_gemm_args* a, hipStream_t st, const cara_g8_plan& plan, const cara_g8_riders* ts);

// helper waves on (CARA_GEMM8_HELPERS=1 or the debug setter; off by default): only then does a riding product write one slab per WAVE
bool cara_gemm8_helpers_on();

// the front end's policy (gemm.hip): does a product of this shape go to the tile?  riders: the launch carries transposed skinny
// products.  (Callers that choose activation layouts ask.)
bool cara_gemm8_policy(int M, int N, int K, int riders);

// skinny.hip: cara_tskinny_partial2_r at rank <= 16, Rp = 32 with a two-stage ring (40 KiB per block)
int cara_tskinny_partial2_small(const void* Xa, int ldxa, const void* Gta, void* slabs_a, int K1a, const void* Xb, int ldxb, const void* Gtb,
                                void* slabs_b, int K1b, int want_colsum_b, int ldg, int M, int Rp, int rank, void* stream);
