// wgrad.h -- long-contraction weight-gradient GEMM (wgrad.hip): C[M,N] += A[K,M]^T . B[K,N], K = T*B rows; bf16 operands
// (T = u16) or f32 operands on the exact-f32 MFMA (T = float), f32 accumulation.
#pragma once
#include "common.h"

namespace fh {

template <class T>
struct WgProblemT {
  const T* A;  // [K, lda], contraction index is the ROW (dgates: k = t*B + b, m = gate column)
  const T* B;  // [K, ldb] (hidden states / inputs: n = feature column)
  float* C;    // [M, ldc] f32, accumulated with atomics
  int64_t lda, ldb, ldc;
  int M, N, K;
  // filled by launch_wgrad
  int m_tiles, n_tiles, splitk, ksteps_per;
  int shared_c;  // another problem of the same launch accumulates into the same C: atomics even without a K split
  int a_col0;    // A points a_col0 columns INTO the rows of its buffer (a column slice): the buffer ends that much earlier
};
using WgProblem = WgProblemT<u16>;
using WgProblem32 = WgProblemT<float>;

// alignment / range preconditions of the kernel (16-byte LDS-DMA pieces, 32-bit buffer offsets)
template <class T>
bool wgrad_eligible(const WgProblemT<T>& p);
// any number of eligible problems: grouped by tile class, split over K so that one launch fills the chip once
template <class T>
int launch_wgrad(const WgProblemT<T>* ps, int n, hipStream_t st);

}  // namespace fh
