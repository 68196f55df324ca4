// disc_mfma.h -- argument block and launches of the matrix-core K5 kernels (disc_mfma.hip: exact-f32 MFMA; disc_lp.hip: bf16
// MFMA with split operands, the bf16 compute mode).  disc.hip decides which one runs and fills the block.
#pragma once
#include "common.h"

namespace fh {

struct DiscMfmaArgs {
  const float* X;  // stationary [NX, D]
  const float* Y;  // streamed   [NY, D]
  int NX, NY;
  float c;
  int x_is_query;
  const int64_t* idx;  // per QUERY target row (global); query b hits local row idx[b] - row0
  int64_t row0;
  const float* rmax;   // per query (MODE 1)
  const float* rsum;
  const float* gsc;    // device scalar
  float gmul;
  float2* part;        // MODE 0: [nchunks][NX]
  float* G;            // MODE 1: [NX, D] accumulated with atomics
  // MODE 2 (one pass, no atomics): G = partials [chunks][NX, D] of the stationary side's gradient; the streamed side's
  // G2 = [x-tiles][NY, D] partial sums of w[y,x] X[x] and WY = [x-tiles][NY] of w[y,x] (reduced by disc.hip's kernels)
  float* G2;
  float* WY;
  int chunk;           // streamed vectors per workgroup (multiple of 64)
};

// mode 0: forward; 1: one gradient (of the stationary side); 2: both (queries stationary).  D = 16 or 32
void disc_f32_launch(const DiscMfmaArgs& a, int D, int mode, dim3 grid, hipStream_t st);
// D = 32 only
void disc_lp_launch(const DiscMfmaArgs& a, int mode, dim3 grid, hipStream_t st);

}  // namespace fh
