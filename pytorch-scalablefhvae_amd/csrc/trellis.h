// trellis.h -- the device code the sequence-trellis satellites share: ctc.hip, falign.hip, ctcbeam.hip, viterbi.hip.
//
// Every function is defined once, here.  What the four files state about their arithmetic holds for these expressions too:
// the including file sets `#pragma clang fp contract(off)` before it includes this header and is built with
// -ffp-contract=off (the header itself holds no product, so there is nothing to fuse).
//
//   batch rules      tr_utt_ok, tr_utt_entry_ok, tr_check_kernel (utt_ptr), tr_label_check_kernel (utt_ptr, lab_ptr, cell_ptr)
//   a frame's row    tr_load_row (lane c owns the classes c and c + 64), tr_log_softmax (butterfly maximum, butterfly float64 sum)
//   log-sum-exp      tr_lse2, tr_lse3 (branch-free)
//   label trellis    tr_num_states, tr_cells, tr_states_per_lane, tr_load_labels, tr_cells_fit,
//                    tr_state_classes (cls / pen of a lane's NS states), tr_left (the two left neighbours across lanes)
//
// The check kernels are templates on the status bit they raise and `static`: the four files are linked into one library
// without relocatable device code, so every translation unit carries its own copy and none is visible to another.
#pragma once

#include <math.h>

#include "common.h"

namespace fh {

constexpr int kTrMaxClasses = 128;  // a lane owns two classes
constexpr int kTrMaxLabels = 256;   // 2 L + 1 <= 513 states: a lane owns at most nine

static_assert(2 * kTrMaxLabels + 1 <= 64 * 9, "a lane owns at most nine states");

// ------------------------------------------------------------------------------------------------------------- batch rules
// the rows [a, b) of an utterance: inside the n_frames rows, at most 2^31 - 1 of them
__device__ __forceinline__ bool tr_utt_ok(int64_t a, int64_t b, int64_t n_frames) {
  return a >= 0 && b >= a && b <= n_frames && b - a <= 0x7fffffffLL;
}

// entry t of a (U + 1,) utt_ptr: the range rule, the first entry 0, the last entry n_frames; a, b: the utterance's rows
__device__ __forceinline__ bool tr_utt_entry_ok(const int64_t* __restrict__ utt_ptr, int64_t t, int64_t U, int64_t n_frames, int64_t& a,
                                                int64_t& b) {
  a = utt_ptr[t], b = utt_ptr[t + 1];
  bool ok = tr_utt_ok(a, b, n_frames);
  if (t == 0) ok = ok && a == 0;
  if (t == U - 1) ok = ok && b == n_frames;
  return ok;
}

// one thread per utterance: the rules of the header; BAD is the file's *_BAD_PTR
template <int BAD>
static __global__ void tr_check_kernel(const int64_t* __restrict__ utt_ptr, int64_t U, int64_t n_frames, int32_t* status) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < U) {
    int64_t a, b;
    if (!tr_utt_entry_ok(utt_ptr, t, U, n_frames, a, b)) atomicOr(status, BAD);
  }
}

// the trellis states of a transcription of L labels: 2 L + 1 with the blank between the labels (ctc), else one per label
__device__ __forceinline__ int64_t tr_num_states(int64_t L, bool ctc) { return ctc ? 2 * L + 1 : L; }

// the workspace cells utterance (T, L) needs: T S; an over-long transcription is refused and needs none
__device__ __forceinline__ int64_t tr_cells(int64_t T, int64_t L, bool ctc) { return L > kTrMaxLabels ? 0 : T * tr_num_states(L, ctc); }

// one thread per utterance: the rules of the header for utt_ptr, lab_ptr and (if given) cell_ptr into a workspace of ws_cells
template <int BAD>
static __global__ void tr_label_check_kernel(const int64_t* __restrict__ utt_ptr, const int64_t* __restrict__ lab_ptr,
                                             const int64_t* __restrict__ cell_ptr, int64_t U, int64_t n_frames, bool ctc,
                                             int64_t ws_cells, int32_t* status) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < U) {
    int64_t a, b;
    const int64_t la = lab_ptr[t], lb = lab_ptr[t + 1];
    bool ok = tr_utt_entry_ok(utt_ptr, t, U, n_frames, a, b) && la >= 0 && lb >= la;
    if (t == 0) ok = ok && la == 0;
    if (ok && cell_ptr != nullptr) {
      const int64_t c0 = cell_ptr[t], c1 = cell_ptr[t + 1];
      ok = c0 >= 0 && c1 >= c0 && c1 <= ws_cells && c1 - c0 >= tr_cells(b - a, lb - la, ctc);
      if (t == 0) ok = ok && c0 == 0;
    }
    if (!ok) atomicOr(status, BAD);
  }
}

// ----------------------------------------------------------------------------------------------------------- a frame's row
__device__ __forceinline__ void tr_load_row(const float* row, int C, int lane, float& z0, float& z1) {
  z0 = lane < C ? row[lane] : -INFINITY;
  z1 = lane + 64 < C ? row[lane + 64] : -INFINITY;
}

// the row's log-softmax: l0, l1 of the lane's classes and lg = log sum exp(z - max) (the largest entry of the row is 0 - lg).
// Every lane computes the same maximum and the same float64 sum, so every lane of every wave that calls it ends with the same lg
struct TrLogSoftmax {
  double l0, l1, lg;
};
__device__ __forceinline__ TrLogSoftmax tr_log_softmax(float z0, float z1) {
  float m = fmaxf(z0, z1);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  const double d0 = (double)z0 - (double)m, d1 = (double)z1 - (double)m;
  double s = exp(d0) + exp(d1);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
  const double lg = log(s);
  return {d0 - lg, d1 - lg, lg};
}

// ------------------------------------------------------------------------------------------------------------- log-sum-exp
// lse of two or three values, branch-free: with every value -inf the maximum is replaced by 0, the sum is 0 and log gives -inf
__device__ __forceinline__ double tr_lse2(double a, double b) {
  const double m = fmax(a, b), mm = m == -INFINITY ? 0.0 : m;
  return mm + log(exp(a - mm) + exp(b - mm));
}
__device__ __forceinline__ double tr_lse3(double a, double b, double c) {
  const double m = fmax(fmax(a, b), c), mm = m == -INFINITY ? 0.0 : m;
  return mm + log(exp(a - mm) + exp(b - mm) + exp(c - mm));
}

// ----------------------------------------------------------------------------------------------------------- label trellis
// One wavefront per utterance; lane l owns the NS contiguous states l NS .. l NS + NS - 1, NS = 1, 2, 4 or 9 by S.

// the states a lane owns for a trellis of S states over L labels (a refused transcription goes with the smallest)
__device__ __forceinline__ int tr_states_per_lane(int64_t L, int64_t S) {
  return (L > kTrMaxLabels || S <= 64) ? 1 : (S <= 128 ? 2 : (S <= 256 ? 4 : 9));
}

// (The kernels compare it with their NS directly after they have read the utterance's pointers, "belongs to another launch:
// return": from that comparison the compiler knows the range of L in each instantiation and shapes the loops over the labels
// by it.  Routed through a struct that holds the utterance, that knowledge was lost and the code of the sweeps changed; so
// the dozen lines that read the pointers stay in the two kernels.)

// the L <= kTrMaxLabels labels from labels[l0 ..) into lab[0 .. L) (LDS; the caller's barrier publishes them).  True, the same in
// all lanes, if one of them lies outside the C classes or is the blank
__device__ __forceinline__ bool tr_load_labels(const int32_t* __restrict__ labels, int64_t l0, int L, int C, int blank, int lane,
                                               int* lab) {
  bool bad = false;
  for (int i = lane; i < L; i += 64) {
    const int v = labels[l0 + i];
    bad = bad || v < 0 || v >= C || v == blank;
    lab[i] = v;
  }
  return __any(bad);
}

// whether the T S cells of an utterance that begin at c0 lie inside a workspace of ws_cells
__device__ __forceinline__ bool tr_cells_fit(int64_t c0, int T, int S, int64_t ws_cells) {
  return !(c0 < 0 || c0 > ws_cells || (int64_t)T * S > ws_cells - c0);
}

// cls: the class of each of the lane's states; a state past the end gets `sentinel`, the index of a -inf entry of the frame's
// row buffer, so that its value is -inf with no test in the step loop.  pen: 0 where the skip into the state (from s - 2) is
// allowed, else -inf (added to the candidate: exact).  ctc: the states are blank, l_0, blank, l_1 .. blank; else l_0, l_1 ..
template <int NS>
__device__ __forceinline__ void tr_state_classes(const int* lab, int lane, int S, bool ctc, int blank, int sentinel, int (&cls)[NS],
                                                 double (&pen)[NS]) {
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = lane * NS + k, li = (s - 1) >> 1;
    const bool odd = ctc && s < S && (s & 1);
    cls[k] = s < S ? (ctc ? (odd ? lab[li] : blank) : lab[s]) : sentinel;
    pen[k] = (odd && s >= 3 && lab[li] != lab[li - 1]) ? 0.0 : -INFINITY;
  }
}

// the values of the states lane NS - 1 (up1) and lane NS - 2 (up2), the two left of the lane's first; -inf before state 0
template <int NS>
__device__ __forceinline__ void tr_left(const double (&a)[NS], int lane, double& up1, double& up2) {
  up1 = __shfl_up(a[NS - 1], 1, 64);
  up2 = NS >= 2 ? __shfl_up(a[NS >= 2 ? NS - 2 : 0], 1, 64) : __shfl_up(a[0], 2, 64);
  if (lane < 1) up1 = -INFINITY;
  if (lane < (NS >= 2 ? 1 : 2)) up2 = -INFINITY;
}

}  // namespace fh
