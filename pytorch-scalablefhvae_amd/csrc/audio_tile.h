// audio_tile.h -- what the audio kernels share (feats, kaldi_fbank, synth, resample; melinv takes the launch side only).
//
// The scheme: a workgroup of 4 waves takes BM = 16 * TM consecutive rows (frames, resampler rows) and gathers them into LDS,
// one row per LDS row of LDA = K + 4 floats (a stride that is an odd multiple of 16 bytes: the 16 rows of a ds_read_b128
// fragment hit 16 distinct bank slots).  A dense product rows . basis^T then runs on the exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32).  Each wave owns whole 16-row groups of the basis for all BM rows: the basis fragment a lane
// loads is reused over the TM row tiles in registers, and no two waves read the same basis rows, so the basis goes from L2
// straight into registers, one 16-k chunk ahead, instead of through LDS.
//
// Every product of the audio pipeline is tile_product below, so every output element is the same fixed-order f32 chain
// (chunk, then k-step, then lane group: the MFMA order) in every kernel.  The bitwise links between the kernels (batch
// invariance, synthesize_mel == synthesize(mel_to_spec), features of resampled audio == the two-step path) rest on that:
// a change to the order lands here, for all of them at once.
//
// The gathers, the epilogues and the *_check_kernel rules differ between the kernels for real reasons and stay with them.
#pragma once
#include <type_traits>

#include "common.h"

namespace fh {

constexpr int kCuLdsBytes = 163840;  // 160 KiB per CU on gfx950; one workgroup may use all of it

// last u in [0, U) with ptr[u] <= x (0 when there is none): the utterance of row / sample x
__device__ __forceinline__ int64_t last_le(const int64_t* ptr, int64_t U, int64_t x) {
  int64_t lo = 0, hi = U - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (ptr[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// acc[t] += B-fragment . A-fragment over one 16-k chunk (SWAP order: lane (i, q) ends with rows 4q..4q+3 of the B side
// (basis rows: bins, mels, samples, bank columns) for column i (row i of the t-th 16-row tile of A))
template <int TM>
__device__ __forceinline__ void mfma_chunk(f32x4 (&acc)[TM], const uint4& b, const uint4 (&a)[TM]) {
  const float bs[4] = {__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z), __uint_as_float(b.w)};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      const float as = s == 0 ? __uint_as_float(a[t].x) : s == 1 ? __uint_as_float(a[t].y) : s == 2 ? __uint_as_float(a[t].z) : __uint_as_float(a[t].w);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(bs[s], as, acc[t], 0, 0, 0);
    }
  }
}

// acc[n][t] += basis stream n . row tile t over the 16-k chunks c = from, from + step, ... (to excluded), in that order.
// b[n]: the lane's basis row of stream n in global memory (+ 4q); ar: the lane's row of the first tile in LDS (+ 4q), the
// t-th tile 16 * LDA floats further.  The NS streams (1; 2 for cos and sin) share one set of row fragments.  The next
// chunk's fragments are loaded before this chunk's products; within a chunk stream 0 comes wholly before stream 1.
// The range must not be empty: chunk `from` is loaded before the loop looks at `to`.
template <int TM, int NS>
__device__ __forceinline__ void tile_product(f32x4 (&acc)[NS][TM], const float* const (&b)[NS], const float* ar, int LDA, int from,
                                             int to, int step) {
  const auto more = [&](int c) { return step > 0 ? c < to : c > to; };
  uint4 nb[NS], na[TM];
#pragma unroll
  for (int n = 0; n < NS; ++n) nb[n] = *(const uint4*)(b[n] + 16 * from);
#pragma unroll
  for (int t = 0; t < TM; ++t) na[t] = *(const uint4*)(ar + t * 16 * LDA + 16 * from);
  for (int c = from; more(c); c += step) {
    uint4 cb[NS], ca[TM];
#pragma unroll
    for (int n = 0; n < NS; ++n) cb[n] = nb[n];
#pragma unroll
    for (int t = 0; t < TM; ++t) ca[t] = na[t];
    if (more(c + step)) {
#pragma unroll
      for (int n = 0; n < NS; ++n) nb[n] = *(const uint4*)(b[n] + 16 * (c + step));
#pragma unroll
      for (int t = 0; t < TM; ++t) na[t] = *(const uint4*)(ar + t * 16 * LDA + 16 * (c + step));
    }
#pragma unroll
    for (int n = 0; n < NS; ++n) mfma_chunk<TM>(acc[n], cb[n], ca);
  }
}

// ---- host side
// the row-tile heights TM a file's kernels are instantiated for, widest first
template <int... TMS>
struct TmSet {
  // the first TM whose tile fits: lds_bytes(BM) <= limit; 0: none does
  template <class F>
  static int largest(int64_t limit, F lds_bytes) {
    int tm = 0;
    (void)((lds_bytes(16 * TMS) <= limit ? (tm = TMS, true) : false) || ...);
    return tm;
  }
  // f(std::integral_constant<int, TM>()) for the run-time tm (one that largest() returned)
  template <class F>
  static int dispatch(int tm, F f) {
    int rc = FHVAE_ERR_LIMIT;
    (void)((tm == TMS ? (rc = f(std::integral_constant<int, TMS>()), true) : false) || ...);
    return rc;
  }
};

// a kernel with `smem` bytes of dynamic LDS: raise the attribute, launch, return the launch status
template <class... P, class... Args>
static inline int launch_lds(void (*fn)(P...), int64_t grid, int threads, int64_t smem, hipStream_t s, Args... args) {
  hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(threads), (size_t)smem, s, args...);
  return fh_launch_status();
}

}  // namespace fh
