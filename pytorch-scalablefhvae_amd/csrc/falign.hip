// falign.hip -- forced alignment on per-frame scores (include/fhvae_falign.h):
//   fhvae_fa_align : the best path of every utterance through the trellis of its transcription, its score and the token times
//
// One wavefront per utterance, as ctc.hip: the recursion is sequential in t and parallel over the S trellis states (2 L + 1 in
// CTC topology, L in HMM topology).  Lane l owns the NS contiguous states l NS .. l NS + NS - 1 (NS = 1, 2, 4 or 9 by S: one
// kernel each), delta in float64 registers; the two left neighbours of a lane's first states arrive by cross-lane moves.  The
// frame's f32 row is loaded two frames ahead and parked in a two-frame LDS buffer a frame ahead, and every state gathers its
// score for the NEXT frame from there while this frame's maxima are taken: the dependent chain of a frame is the cross-lane
// moves, two compares and one addition.  A state past the end reads a -inf entry, and the skip rule is an additive 0 / -inf
// penalty, so the step loop holds no per-state test.
//
// BACK-POINTERS.  Two bits per state, a lane's NS codes packed into ONE store per frame: a byte per lane (NS = 2, 4: 64 bytes a
// frame), a dword per lane (NS = 9: 256 bytes a frame), or a byte per state (NS = 1: S bytes a frame).  Frame 0 has none.  That
// is never more than the T S bytes the header grants an utterance.
//
// TRACE-BACK.  The packed rows of 64 frames are brought into LDS side by side (whole rows: at most 16 KB, so no window around q
// is needed), one lane walks them there (a dependent LDS read per frame, not a dependent global read), and the wave stores the
// 64 state entries side by side.  The same lanes write seg: frame t begins (ends) label i when the frame before (after) sits in
// another state; the neighbours across a chunk edge are carried in a register and one LDS word.  No atomics but the status word.
//
// Arithmetic: the header's expressions as written (the pragma below and -ffp-contract=off; there is nothing to fuse).
#pragma clang fp contract(off)

#include <math.h>

#include "common.h"
#include "trellis.h"

#include "../../include/fhvae_falign.h"

namespace fh {

constexpr int kFaCP = FHVAE_FA_MAX_CLASSES;  // entry kFaCP of each half of FaLds::z is -inf
constexpr int kFaZP = kFaCP + 4;             // a half of the row buffer
constexpr int kFaFrames = 64;                // frames per trace-back chunk

static_assert(FHVAE_FA_MAX_CLASSES == kTrMaxClasses && FHVAE_FA_MAX_LABELS == kTrMaxLabels, "the lane layout of trellis.h");

// bytes of a frame's packed back-pointers, at most (NS = 1: S <= 64 of them)
template <int NS>
constexpr int fa_max_row_bytes() {
  return NS == 9 ? 256 : 64;
}

template <int NS>
struct FaLds {
  float z[2 * kFaZP];                                         // the rows of two frames; entry kFaCP of each half is -inf
  int lab[FHVAE_FA_MAX_LABELS];
  uint32_t bp[kFaFrames * fa_max_row_bytes<NS>() / 4 + 2];    // the packed back-pointers of a chunk (and up to 3 bytes before)
  int qs[kFaFrames];                                          // the chunk's states
  double fin[2];                                              // delta_{T-1} of S - 1 and S - 2
  int qedge;                                                  // the state of the frame before the chunk
};

// NS: the states a lane owns.  The call launches the kernel once per NS and a workgroup whose utterance belongs to another NS
// returns at once, as ctc.hip.
template <int NS>
__global__ void __launch_bounds__(64)
    fa_align_kernel(const float* __restrict__ scores, int64_t lds, int64_t n_frames, int C, int blank,
                    const int64_t* __restrict__ utt_ptr, const int32_t* __restrict__ labels, const int64_t* __restrict__ lab_ptr,
                    const int64_t* __restrict__ cell_ptr, int64_t U, int32_t* __restrict__ state, int32_t* __restrict__ seg,
                    double* __restrict__ score, int32_t* status, uint8_t* ws, int64_t ws_bytes) {
  __shared__ FaLds<NS> sm;
  if (*status & FHVAE_FA_BAD_PTR) return;  // (set by the check kernel)
  const int lane = threadIdx.x;
  // ---- the utterance.  Everything up to the first barrier is the same in all lanes: they return together or not at all
  const int64_t u = blockIdx.x;
  if (u >= U || C < 2 || C > kFaCP || blank < -1 || blank >= C) return;
  const int64_t u0 = utt_ptr[u], u1 = utt_ptr[u + 1], l0 = lab_ptr[u], l1 = lab_ptr[u + 1];
  if (!tr_utt_ok(u0, u1, n_frames) || l0 < 0 || l1 < l0) return;
  const int T = (int)(u1 - u0);
  const int64_t L64 = l1 - l0;
  const bool ctc = blank >= 0;
  if (tr_states_per_lane(L64, tr_num_states(L64, ctc)) != NS) return;
  int bits = 0;
  int L = 0;
  if (L64 > FHVAE_FA_MAX_LABELS) {
    bits = FHVAE_FA_BAD_LABEL;
  } else {
    L = (int)L64;
    if (tr_load_labels(labels, l0, L, C, blank, lane, sm.lab)) bits = FHVAE_FA_BAD_LABEL;
  }
  const int S = (int)tr_num_states(L, ctc);
  const int rs = NS == 1 ? S : fa_max_row_bytes<NS>();  // bytes of a frame's back-pointers
  int64_t bp0 = 0;                                       // where the utterance's back-pointers begin in ws
  if (bits == 0 && T > 0) {
    const int64_t c0 = cell_ptr[u];
    if (!tr_cells_fit(c0, T, S, ws_bytes)) return;  // (the check kernel has refused this already; a cell is a byte)
    bp0 = NS == 9 ? (c0 + 3) & ~(int64_t)3 : c0;  // (T - 1) rs + 3 <= T S for S >= 257: the dword stores stay in the utterance's bytes
  }
  for (int64_t i = lane; i < 2 * L64; i += 64) seg[2 * l0 + i] = -1;

  double best = -INFINITY;
  int q = 0;
  if (bits == 0 && T == 0) {
    if (L == 0) best = 0.0;
  } else if (bits == 0 && S > 0) {
    __syncthreads();
    // cls, pen: trellis.h; a state past the end reads the -inf entry of z, so its delta is -inf with no test in the loop
    int cls[NS];
    double pen[NS];
    tr_state_classes<NS>(sm.lab, lane, S, ctc, blank, kFaCP, cls, pen);
    if (lane == 0) sm.z[kFaCP] = -INFINITY, sm.z[kFaZP + kFaCP] = -INFINITY;
    const float* z = scores + u0 * lds;
    // ---- forward.  n0, n1: the row two frames ahead at the top of the loop; e: this frame's scores of the lane's states
    float n0, n1;
    tr_load_row(z, C, lane, n0, n1);
    sm.z[lane] = n0, sm.z[lane + 64] = n1;
    if (T > 1) tr_load_row(z + lds, C, lane, n0, n1);
    __syncthreads();
    double a[NS];
    float e[NS];
    const int n_start = ctc ? 2 : 1;
#pragma unroll
    for (int k = 0; k < NS; ++k) a[k] = lane * NS + k < n_start ? (double)sm.z[cls[k]] : -INFINITY;
    if (T > 1) {
      sm.z[kFaZP + lane] = n0, sm.z[kFaZP + lane + 64] = n1;
      if (T > 2) tr_load_row(z + 2 * lds, C, lane, n0, n1);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NS; ++k) e[k] = sm.z[kFaZP + cls[k]];
    uint8_t* row = ws + bp0;
    for (int t = 1; t < T; ++t) {
      float* zn = sm.z + ((t + 1) & 1) * kFaZP;
      if (t + 1 < T) {
        zn[lane] = n0, zn[lane + 64] = n1;
        if (t + 2 < T) tr_load_row(z + (int64_t)(t + 2) * lds, C, lane, n0, n1);  // two frames ahead
      }
      __syncthreads();
      float en[NS];
#pragma unroll
      for (int k = 0; k < NS; ++k) en[k] = zn[cls[k]];  // the next frame's scores: not needed before the next turn
      double up1, up2;
      tr_left<NS>(a, lane, up1, up2);
      uint32_t code = 0;
#pragma unroll
      for (int k = NS - 1; k >= 0; --k) {  // downwards: a[k - 1] and a[k - 2] are still the frame before's
        const double p1 = k >= 1 ? a[k >= 1 ? k - 1 : 0] : up1;
        const double p2 = (k >= 2 ? a[k >= 2 ? k - 2 : 0] : (k == 1 ? up1 : up2)) + pen[k];
        double m = a[k];
        uint32_t b = 0;
        if (p1 > m) m = p1, b = 1;
        if (p2 > m) m = p2, b = 2;
        a[k] = m + (double)e[k];
        code |= b << (2 * k);
      }
      if (NS == 1) {
        if (lane < S) row[lane] = (uint8_t)code;
      } else if (NS == 9) {
        ((uint32_t*)row)[lane] = code;
      } else {
        row[lane] = (uint8_t)code;
      }
      row += rs;
#pragma unroll
      for (int k = 0; k < NS; ++k) e[k] = en[k];
    }
    // ---- the end state
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int s = lane * NS + k;
      if (s == S - 1) sm.fin[0] = a[k];
      if (s == S - 2) sm.fin[1] = a[k];
    }
    __syncthreads();
    const double v1 = sm.fin[0], v2 = (ctc && L >= 1) ? sm.fin[1] : -INFINITY;
    best = v2 > v1 ? v2 : v1;
    q = v2 > v1 ? S - 2 : S - 1;
  }
  if (bits == 0 && best == -INFINITY) bits = FHVAE_FA_INFEASIBLE;
  if (bits != 0) {  // no path: -inf and -1 (seg holds -1 already)
    for (int i = lane; i < T; i += 64) state[u0 + i] = -1;
    if (lane == 0) score[u] = -INFINITY, atomicOr(status, bits);
    return;
  }
  if (lane == 0) score[u] = best;

  // ---- trace-back, 64 frames at a time from the end.  Frame t's back-pointers are row t - 1
  int qnext = -1;  // the state of the frame after the chunk
  for (int hi = T; hi > 0; hi -= kFaFrames) {
    const int lo = hi > kFaFrames ? hi - kFaFrames : 0, nf = hi - lo;
    const int r0 = (lo > 0 ? lo : 1) - 1;                   // the rows r0 .. hi - 2
    const int64_t g0 = bp0 + (int64_t)r0 * rs, g4 = g0 & ~(int64_t)3;
    const int shift = (int)(g0 - g4), ndw = (shift + (hi - 1 - r0) * rs + 3) >> 2;
    __syncthreads();  // the forward's stores are visible to the wave; the chunk before is consumed
    for (int i = lane; i < ndw; i += 64) {
      const int64_t off = g4 + 4 * (int64_t)i;
      uint32_t v = 0;
      if (off + 4 <= ws_bytes) {
        v = *(const uint32_t*)(ws + off);
      } else {
        for (int j = 0; j < 4; ++j)
          if (off + j < ws_bytes) v |= (uint32_t)ws[off + j] << (8 * j);
      }
      sm.bp[i] = v;
    }
    __syncthreads();
    if (lane == 0) {
      const uint8_t* bb = (const uint8_t*)sm.bp + shift;
      for (int t = hi - 1; t >= lo; --t) {
        sm.qs[t - lo] = q;
        if (t > 0) {
          const uint8_t* r = bb + (t - 1 - r0) * rs;
          uint32_t b;
          if (NS == 1) b = r[q];
          else if (NS == 2) b = r[q >> 1] >> (2 * (q & 1));
          else if (NS == 4) b = r[q >> 2] >> (2 * (q & 3));
          else b = ((const uint32_t*)r)[q / 9] >> (2 * (q % 9));  // (bp0 is a multiple of 4 here: shift is 0)
          b &= 3;
          q -= b > 2 ? 2 : (int)b;  // clamped: whatever the bytes hold, q stays in [0, S)
          q = q < 0 ? 0 : q;
        }
      }
      sm.qedge = q;
    }
    __syncthreads();
    if (lane < nf) {
      const int t = lo + lane, qi = sm.qs[lane];
      state[u0 + t] = qi;
      const int prev = lane > 0 ? sm.qs[lane - 1] : (lo > 0 ? sm.qedge : -1);
      const int next = lane < nf - 1 ? sm.qs[lane + 1] : qnext;
      const int li = ctc ? qi >> 1 : qi;
      if ((!ctc || (qi & 1)) && li < L) {
        if (prev != qi) seg[2 * (l0 + li)] = t;
        if (next != qi) seg[2 * (l0 + li) + 1] = t;
      }
    }
    qnext = sm.qs[0];
  }
}

static inline int64_t fa_ws(int64_t cells) { return (cells + 255) / 256 * 256; }

}  // namespace fh

using namespace fh;

extern "C" int64_t fhvae_fa_ws_bytes(int64_t cells) {
  if (cells < 0 || cells > (1LL << 59)) return 0;
  return fa_ws(cells);
}

extern "C" int fhvae_fa_align(const float* scores, int64_t lds, int64_t n_frames, int64_t C, int64_t blank, const int64_t* utt_ptr,
                              const int32_t* labels, const int64_t* lab_ptr, const int64_t* cell_ptr, int64_t U, int32_t* state,
                              int32_t* seg, double* score, int32_t* status, void* ws, int64_t ws_bytes, void* stream) {
  FH_CHECK_PTR(status);
  if (C < 2 || blank < -1 || blank >= C || n_frames < 0 || U < 0 || lds < C || ws_bytes < 0) return FHVAE_ERR_SHAPE;
  if (C > FHVAE_FA_MAX_CLASSES || n_frames > (1LL << 52)) return FHVAE_ERR_LIMIT;
  FH_CHECK_I32(U);
  if (U == 0) return FHVAE_OK;
  FH_CHECK_PTR(scores);
  FH_CHECK_PTR(utt_ptr);
  FH_CHECK_PTR(labels);
  FH_CHECK_PTR(lab_ptr);
  FH_CHECK_PTR(cell_ptr);
  FH_CHECK_PTR(state);
  FH_CHECK_PTR(seg);
  FH_CHECK_PTR(score);
  FH_CHECK_PTR(ws);
  if (lds % 4 != 0 || ((uintptr_t)scores & 15) != 0 || ((uintptr_t)ws & 15) != 0) return FHVAE_ERR_ALIGN;
  if (((uintptr_t)utt_ptr & 7) != 0 || ((uintptr_t)labels & 3) != 0 || ((uintptr_t)lab_ptr & 7) != 0 || ((uintptr_t)cell_ptr & 7) != 0 ||
      ((uintptr_t)state & 3) != 0 || ((uintptr_t)seg & 3) != 0 || ((uintptr_t)score & 7) != 0 || ((uintptr_t)status & 3) != 0)
    return FHVAE_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tr_label_check_kernel<FHVAE_FA_BAD_PTR>, dim3((unsigned)fh_cdiv(U, 256)), dim3(256), 0, st, utt_ptr, lab_ptr,
                     cell_ptr, U, n_frames, blank >= 0, ws_bytes, status);  // (a back-pointer cell is one byte)
#define FA_LAUNCH(NS)                                                                                                           \
  hipLaunchKernelGGL(fa_align_kernel<NS>, dim3((unsigned)U), dim3(64), 0, st, scores, lds, n_frames, (int)C, (int)blank, utt_ptr, \
                     labels, lab_ptr, cell_ptr, U, state, seg, score, status, (uint8_t*)ws, ws_bytes)
  FA_LAUNCH(1);
  FA_LAUNCH(2);
  FA_LAUNCH(4);
  FA_LAUNCH(9);
#undef FA_LAUNCH
  return fh_launch_status();
}
