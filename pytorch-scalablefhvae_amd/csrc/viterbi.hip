// viterbi.hip -- phone recognition on per-frame scores (include/fhvae_viterbi.h):
//   fhvae_vit_decode : the best state sequence of every utterance under a dense (C, C) transition table
//   fhvae_edit_align : substitutions, deletions, insertions and correct tokens of every (ref, hyp) pair
//
// DECODER.  Per frame the work is a max-plus product of the C-vector d with the (C, C) table: sequential in t, parallel over the
// target state c, the source state p and the utterances.  The table sits in LDS as (p, c) with c contiguous and the row padded
// to 64 or 128 words, so that the lanes, which own the target states c = lane (and lane + 64 when C > 64), read consecutive
// words of row p: no bank conflict.  d lives in registers; d[p] reaches every lane as a lane read with a wave-uniform index
// (v_readlane_b32), which costs no LDS traffic.  The running best is a (value, index) pair and p is met in increasing order
// with a strict comparison, so the smallest p of equal values wins.
// One workgroup of four waves per utterance, each wave scanning a quarter of p (see vit_decode_kernel).  The frame's emission
// row is loaded one frame ahead of its use; the back-pointers go to the workspace as one byte per (frame, state),
// lane-contiguous.  The trace-back reuses the table's LDS: the workgroup loads the
// back-pointers of 64 frames side by side, one thread walks them in LDS (a dependent LDS read per frame instead of a dependent
// global read), and the workgroup stores the 64 path entries side by side.
//
// ALIGNER.  One wavefront per pair, one anti-diagonal sweep over the whole hyp, as abx.hip / qbe.hip: lane l owns the four ref
// rows 4 l + 1 .. 4 l + 4 and at step t computes their cells of hyp column t - l, top to bottom; the cell above its first row is
// lane l - 1's last row of the same column (one shuffle, computed a step earlier), the diagonal the shuffle of the step before.
// The hyp streams through a ring of two 64-token tiles in LDS and the sweep never restarts at a tile.  A cell carries (cost,
// S, D) only: along any path S + D + Cor = i and S + I + Cor = j, so I and Cor follow at the end; S and D (at most 256) share a word.
//
// Arithmetic: exactly the header's; every f32 operation is an addition rounded once or a comparison (the pragma below and
// -ffp-contract=off; there is nothing to fuse).  No atomics except the atomicOr of the status word.
#pragma clang fp contract(off)

#include <math.h>

#include "common.h"
#include "trellis.h"

#include "../../include/fhvae_viterbi.h"

namespace fh {

constexpr int kVitFrames = 64;  // frames per trace-back chunk
constexpr int kVitWaves = 4;    // waves of a decoder workgroup: the source states are split over them
constexpr int kVitThreads = 64 * kVitWaves;
constexpr int kEdRows = FHVAE_EDIT_MAX_REF / 64;  // ref rows per lane
constexpr int kEdRing = 128;    // hyp tokens in the ring: two tiles of 64

static_assert(FHVAE_VIT_MAX_STATES == 128, "a lane owns one or two states");
static_assert(kEdRows * 64 == FHVAE_EDIT_MAX_REF && FHVAE_EDIT_MAX_REF < 65536, "S and D share a word, 16 bits each");

__device__ __forceinline__ float vit_lane_read(float v, int p) {  // v of lane p; p is wave-uniform
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), p));
}

// the best predecessor among p0 <= p < p1 (p0 < p1 <= C) for the lane's NS target states: (best, bp) = (v(p0), p0), then every
// later p replaces it only if strictly larger
template <int NS>
__device__ __forceinline__ void vit_scan(const float* tr, const float (&d)[NS], int p0, int p1, int lane, float (&best)[NS],
                                         int (&bp)[NS]) {
  constexpr int CP = 64 * NS;
  {
    const float dp = vit_lane_read(p0 < 64 ? d[0] : d[NS - 1], p0 & 63);
#pragma unroll
    for (int s = 0; s < NS; ++s) best[s] = dp + tr[p0 * CP + lane + 64 * s], bp[s] = p0;
  }
  const int mid = p1 < 64 ? p1 : 64;
  for (int p = p0 + 1; p < mid; ++p) {
    const float dp = vit_lane_read(d[0], p);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const float v = dp + tr[p * CP + lane + 64 * s];
      if (v > best[s]) best[s] = v, bp[s] = p;
    }
  }
  if (NS > 1) {
    for (int p = (p0 + 1 > 64 ? p0 + 1 : 64); p < p1; ++p) {
      const float dp = vit_lane_read(d[NS - 1], p - 64);
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const float v = dp + tr[p * CP + lane + 64 * s];
        if (v > best[s]) best[s] = v, bp[s] = p;
      }
    }
  }
}

// NS: the states a lane owns, 1 (C <= 64) or 2 (C <= 128); it sizes the table in LDS (16 KB or 64 KB).
// The source states are split over the workgroup's four waves: each wave holds all of d, scans its quarter of p and parks its
// (best, index) per target state in LDS; after ONE barrier per frame (the parking slots alternate between two sets, so a wave
// that runs ahead writes the other set) every wave merges the four partials in increasing wave, that is increasing p, with the
// same strict comparison: the bits are those of one scan over all p.  (One wavefront per utterance with no barrier at all was
// built and measured as well: 1.8 to 2.9 times slower in every case)
template <int NS>
__global__ void __launch_bounds__(kVitThreads)
    vit_decode_kernel(const float* __restrict__ emit, int64_t lde, int64_t n_frames, int C, const float* __restrict__ trans,
                      const float* __restrict__ init, const float* __restrict__ fin, const int64_t* __restrict__ utt_ptr, int64_t U,
                      int32_t* __restrict__ path, float* __restrict__ score, const int32_t* status, uint8_t* ws) {
  constexpr int CP = 64 * NS, NT = kVitThreads, NW = kVitWaves;
  __shared__ float tr[CP * CP];  // (p, c) at p * CP + c; the trace-back reuses it for the back-pointers of 64 frames
  __shared__ int qs[kVitFrames];
  __shared__ float rv[2 * NW * CP];  // the waves' partial maxima: (frame parity, wave, c)
  __shared__ int ri[2 * NW * CP];
  if (*status & FHVAE_VIT_BAD_PTR) return;  // (set by the check kernel)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // ---- the utterance.  Everything up to the first barrier is the same in all threads: they return together or not at all
  const int64_t u = blockIdx.x;
  if (u >= U || C < 1 || C > CP) return;
  const int64_t u0 = utt_ptr[u], u1 = utt_ptr[u + 1];
  if (!tr_utt_ok(u0, u1, n_frames)) return;
  const int m = (int)(u1 - u0);
  if (m == 0) {
    if (tid == 0) score[u] = -INFINITY;
    return;
  }
  for (int i = tid; i < C * CP; i += NT) {
    const int p = i / CP, c = i - p * CP;
    tr[i] = c < C ? trans[p * C + c] : 0.f;
  }
  __syncthreads();

  // ---- forward.  A lane's state s is c = lane + 64 s; a lane without a state (c >= C) computes on zeros and stores nothing
  const int quarter = (C + NW - 1) / NW, p0 = wave * quarter, p1 = p0 + quarter < C ? p0 + quarter : C;
  float d[NS], en[NS];
  const float* e = emit + u0 * lde;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int c = lane + 64 * s;
    d[s] = c < C ? init[c] + e[c] : 0.f;
    en[s] = (c < C && m > 1) ? e[lde + c] : 0.f;
  }
  for (int t = 1; t < m; ++t) {
    float ec[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int c = lane + 64 * s;
      ec[s] = en[s];
      en[s] = (c < C && t + 1 < m) ? e[(int64_t)(t + 1) * lde + c] : 0.f;  // the next frame's row flies under this frame's scan
    }
    float best[NS];
    int bp[NS];
    if (p0 < p1) {
      vit_scan<NS>(tr, d, p0, p1, lane, best, bp);
    } else {  // (a wave without a source state: it loses against wave 0's partial, whatever that is)
#pragma unroll
      for (int s = 0; s < NS; ++s) best[s] = -INFINITY, bp[s] = 0;
    }
    const int slot = (t & 1) * NW * CP;
#pragma unroll
    for (int s = 0; s < NS; ++s) rv[slot + wave * CP + lane + 64 * s] = best[s], ri[slot + wave * CP + lane + 64 * s] = bp[s];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      best[s] = rv[slot + lane + 64 * s], bp[s] = ri[slot + lane + 64 * s];
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        const float v = rv[slot + w * CP + lane + 64 * s];
        if (v > best[s]) best[s] = v, bp[s] = ri[slot + w * CP + lane + 64 * s];
      }
    }
    uint8_t* row = ws + (u0 + t) * C;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int c = lane + 64 * s;
      d[s] = best[s] + ec[s];
      if (c < C && wave == 0) row[c] = (uint8_t)bp[s];
    }
  }

  // ---- the end: the smallest c of the largest w.  A lane without a state offers (-inf, c >= C), which loses every tie
  float wv = -INFINITY;
  int wi = lane;
#pragma unroll
  for (int s = NS - 1; s >= 0; --s) {
    const int c = lane + 64 * s;
    const float w = c < C ? (fin != nullptr ? d[s] + fin[c] : d[s]) : -INFINITY;
    if (s == NS - 1 || w >= wv) wv = w, wi = c;  // (the smaller c takes an equal value)
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(wv, o, 64);
    const int i2 = __shfl_xor(wi, o, 64);
    if (v2 > wv || (v2 == wv && i2 < wi)) wv = v2, wi = i2;
  }
  wv = vit_lane_read(wv, 0), wi = __builtin_amdgcn_readlane(wi, 0);
  if (tid == 0) score[u] = wv;

  // ---- trace-back, 64 frames at a time from the end (every wave holds the same d, so thread 0's q is the workgroup's)
  int q = wi < 0 ? 0 : (wi >= C ? C - 1 : wi);
  uint8_t* bb = (uint8_t*)tr;
  for (int hi = m; hi > 0; hi -= kVitFrames) {
    const int lo = hi > kVitFrames ? hi - kVitFrames : 0, nf = hi - lo;
    __syncthreads();  // the forward's stores are visible to the workgroup; the chunk before is consumed
    const uint8_t* src = ws + (u0 + lo) * C;
    for (int i = tid; i < nf * C; i += NT) bb[i] = src[i];
    __syncthreads();
    if (tid == 0) {
      for (int t = hi - 1; t >= lo; --t) {
        qs[t - lo] = q;
        if (t > 0) {  // (frame 0 has no back-pointer: its row of the workspace is never written)
          const int b = bb[(t - lo) * C + q];
          q = b >= C ? C - 1 : b;
        }
      }
    }
    __syncthreads();
    if (tid < nf) path[u0 + lo + tid] = qs[tid];
  }
}

// one thread per pair: the rules of the header
__global__ void edit_check_kernel(const int64_t* __restrict__ ref_ptr, const int64_t* __restrict__ hyp_ptr, int64_t U, int32_t* status) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < U) {
    const int64_t r0 = ref_ptr[t], r1 = ref_ptr[t + 1], h0 = hyp_ptr[t], h1 = hyp_ptr[t + 1];
    bool ok = r0 >= 0 && r1 >= r0 && h0 >= 0 && h1 >= h0 && h1 - h0 <= 0x7fffffffLL;
    if (t == 0) ok = ok && r0 == 0 && h0 == 0;
    if (!ok) atomicOr(status, FHVAE_EDIT_BAD_PTR);
    else if (r1 - r0 > FHVAE_EDIT_MAX_REF) atomicOr(status, FHVAE_EDIT_BAD_REF);
  }
}

__global__ void __launch_bounds__(64)
    edit_align_kernel(const int32_t* __restrict__ ref, const int64_t* __restrict__ ref_ptr, const int32_t* __restrict__ hyp,
                      const int64_t* __restrict__ hyp_ptr, int64_t U, int32_t* __restrict__ counts, const int32_t* status) {
  __shared__ int32_t ring[kEdRing];  // hyp token j at j % 128
  if (*status & FHVAE_EDIT_BAD_PTR) return;  // (set by the check kernel)
  const int lane = threadIdx.x;
  const int64_t u = blockIdx.x;
  if (u >= U) return;
  const int64_t r0 = ref_ptr[u], r1 = ref_ptr[u + 1], h0 = hyp_ptr[u], h1 = hyp_ptr[u + 1];
  if (r0 < 0 || r1 < r0 || h0 < 0 || h1 < h0 || h1 - h0 > 0x7fffffffLL) return;
  int32_t* out = counts + u * 4;
  if (r1 - r0 > FHVAE_EDIT_MAX_REF) {
    if (lane < 4) out[lane] = -1;
    return;
  }
  const int n = (int)(r1 - r0), m = (int)(h1 - h0);
  if (n == 0 || m == 0) {  // all insertions, or all deletions
    if (lane == 0) out[0] = 0, out[1] = n, out[2] = m, out[3] = 0;
    return;
  }
  // the lane's rows i = 4 lane + r + 1; lc / lsd: the cell to the left, [i][0] = i deletions at the start.  sd = S | D << 16
  int tok[kEdRows], lc[kEdRows], lsd[kEdRows];
#pragma unroll
  for (int r = 0; r < kEdRows; ++r) {
    const int i0 = kEdRows * lane + r;
    tok[r] = i0 < n ? ref[r0 + i0] : 0;
    lc[r] = i0 + 1, lsd[r] = (i0 + 1) << 16;
  }
  int dc = kEdRows * lane, dsd = (kEdRows * lane) << 16;  // the diagonal of the first row: [4 lane][j - 1], at the start [4 lane][0]
  const int nl = (n + kEdRows - 1) / kEdRows;             // lanes at work
  const int64_t steps = (int64_t)m + nl - 1;              // (m may be 2^31 - 1: the steps count in int64)
  for (int64_t t0 = 0; t0 < steps; t0 += 64) {
    __syncthreads();  // the steps before have read the tile this one replaces
    if (t0 + lane < m) ring[(t0 + lane) & (kEdRing - 1)] = hyp[h0 + t0 + lane];
    __syncthreads();
    const int64_t t1 = t0 + 64 < steps ? t0 + 64 : steps;
    for (int64_t t = t0; t < t1; ++t) {
      const int upc = __shfl_up(lc[kEdRows - 1], 1, 64);  // [4 lane][j]: lane - 1's last row after step t - 1
      const int upsd = __shfl_up(lsd[kEdRows - 1], 1, 64);
      const int64_t j0 = t - lane;  // the lane's column, from 0
      if (lane < nl && j0 >= 0 && j0 < m) {
        const int h = ring[j0 & (kEdRing - 1)];
        int uc = upc, usd = upsd, gc = dc, gsd = dsd;
        if (lane == 0) uc = (int)j0 + 1, usd = 0, gc = (int)j0, gsd = 0;  // row 0: j insertions
#pragma unroll
        for (int r = 0; r < kEdRows; ++r) {
          const int ne = tok[r] != h ? 1 : 0;
          int bc = gc + ne, bsd = gsd + ne;                            // diagonal: a substitution or a correct token
          if (uc + 1 < bc) bc = uc + 1, bsd = usd + 0x10000;           // up: a deletion
          if (lc[r] + 1 < bc) bc = lc[r] + 1, bsd = lsd[r];            // left: an insertion
          gc = lc[r], gsd = lsd[r];                                    // the next row's diagonal is this row's left
          lc[r] = bc, lsd[r] = bsd;
          uc = bc, usd = bsd;                                          // and its upper cell is this one
        }
      }
      dc = upc, dsd = upsd;
    }
  }
  const int rf = (n - 1) % kEdRows;
  if (lane == (n - 1) / kEdRows) {
    int c = 0, sd = 0;
#pragma unroll
    for (int r = 0; r < kEdRows; ++r)
      if (r == rf) c = lc[r], sd = lsd[r];
    const int S = sd & 0xffff, D = sd >> 16;
    out[0] = S, out[1] = D, out[2] = c - S - D, out[3] = n - S - D;
  }
}

static inline int64_t vit_ws(int64_t n_frames, int64_t C) { return (n_frames * C + 255) / 256 * 256; }

}  // namespace fh

using namespace fh;

extern "C" int64_t fhvae_vit_ws_bytes(int64_t n_frames, int64_t C) {
  if (n_frames < 0 || C < 1 || C > FHVAE_VIT_MAX_STATES || n_frames > INT64_MAX / 256) return 0;
  return vit_ws(n_frames, C);
}

extern "C" int fhvae_vit_decode(const float* emit, int64_t lde, int64_t n_frames, int64_t C, const float* trans, const float* init,
                                const float* fin, const int64_t* utt_ptr, int64_t U, int32_t* path, float* score, int32_t* status,
                                void* ws, int64_t ws_bytes, void* stream) {
  FH_CHECK_PTR(status);
  if (C < 1 || n_frames < 0 || U < 0 || lde < C) return FHVAE_ERR_SHAPE;
  if (C > FHVAE_VIT_MAX_STATES || n_frames > INT64_MAX / 256) return FHVAE_ERR_LIMIT;
  FH_CHECK_I32(U);
  if (U == 0) return FHVAE_OK;
  FH_CHECK_PTR(emit);
  FH_CHECK_PTR(trans);
  FH_CHECK_PTR(init);
  FH_CHECK_PTR(utt_ptr);
  FH_CHECK_PTR(path);
  FH_CHECK_PTR(score);
  FH_CHECK_PTR(ws);
  if (lde % 4 != 0 || ((uintptr_t)emit & 15) != 0) return FHVAE_ERR_ALIGN;
  if (((uintptr_t)trans & 3) != 0 || ((uintptr_t)init & 3) != 0 || ((uintptr_t)fin & 3) != 0 || ((uintptr_t)utt_ptr & 7) != 0 ||
      ((uintptr_t)path & 3) != 0 || ((uintptr_t)score & 3) != 0 || ((uintptr_t)status & 3) != 0)
    return FHVAE_ERR_ALIGN;
  if (ws_bytes < vit_ws(n_frames, C)) return FHVAE_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tr_check_kernel<FHVAE_VIT_BAD_PTR>, dim3((unsigned)fh_cdiv(U, 256)), dim3(256), 0, st, utt_ptr, U, n_frames, status);
  hipLaunchKernelGGL(C <= 64 ? vit_decode_kernel<1> : vit_decode_kernel<2>, dim3((unsigned)U), dim3(kVitThreads), 0, st, emit, lde, n_frames, (int)C, trans, init, fin, utt_ptr, U,
                     path, score, status, (uint8_t*)ws);
  return fh_launch_status();
}

extern "C" int fhvae_edit_align(const int32_t* ref, const int64_t* ref_ptr, const int32_t* hyp, const int64_t* hyp_ptr, int64_t U,
                                int32_t* counts, int32_t* status, void* stream) {
  FH_CHECK_PTR(status);
  if (U < 0) return FHVAE_ERR_SHAPE;
  FH_CHECK_I32(U);
  if (U == 0) return FHVAE_OK;
  FH_CHECK_PTR(ref);
  FH_CHECK_PTR(ref_ptr);
  FH_CHECK_PTR(hyp);
  FH_CHECK_PTR(hyp_ptr);
  FH_CHECK_PTR(counts);
  if (((uintptr_t)ref & 3) != 0 || ((uintptr_t)hyp & 3) != 0 || ((uintptr_t)ref_ptr & 7) != 0 || ((uintptr_t)hyp_ptr & 7) != 0 ||
      ((uintptr_t)counts & 3) != 0 || ((uintptr_t)status & 3) != 0)
    return FHVAE_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(edit_check_kernel, dim3((unsigned)fh_cdiv(U, 256)), dim3(256), 0, st, ref_ptr, hyp_ptr, U, status);
  hipLaunchKernelGGL(edit_align_kernel, dim3((unsigned)U), dim3(64), 0, st, ref, ref_ptr, hyp, hyp_ptr, U, counts, status);
  return fh_launch_status();
}
