// Run-time epilogue -> compile-time epilogue, for the launchers of gemm.hip and gemm8.hip.
#pragma once
#include <type_traits>

#include "common.h"

// A run-time epilogue as a compile-time one: f(std::integral_constant<int, EPI>) for the epilogues in MASK (bit = the CARA_EPI_*
// value), CARA_E_ARG for any other.  Only the epilogues in MASK are instantiated.
constexpr unsigned EPI_MASK_ALL = 0x7f;
constexpr unsigned EPI_MASK_TILE = (1u << CARA_EPI_BF16) | (1u << CARA_EPI_F32) | (1u << CARA_EPI_GELU) | (1u << CARA_EPI_RESID) | (1u << CARA_EPI_DGELU);
template <unsigned MASK, class F>
int cara_dispatch_epi(const int epi, F&& f) {
#define CARA_EPI_CASE(E) \
  case E:                \
    if constexpr ((MASK >> E) & 1u) return f(std::integral_constant<int, E>{}); else break;
  switch (epi) {
    CARA_EPI_CASE(CARA_EPI_BF16)
    CARA_EPI_CASE(CARA_EPI_F32)
    CARA_EPI_CASE(CARA_EPI_GELU)
    CARA_EPI_CASE(CARA_EPI_RESID)
    CARA_EPI_CASE(CARA_EPI_DGELU)
    CARA_EPI_CASE(CARA_EPI_GELU_DG)
    CARA_EPI_CASE(CARA_EPI_MULH)
    default: break;
  }
#undef CARA_EPI_CASE
  return CARA_E_ARG;
}
