// ctc.hip -- connectionist temporal classification on per-frame logits (include/fhvae_ctc.h):
//   fhvae_ctc_loss : nll of every utterance's transcription over all alignments, and its gradient with respect to the logits
//
// One wavefront per utterance; the recursion is sequential in t and parallel over the S = 2 L + 1 trellis states.  Lane l owns the
// NS contiguous states l NS .. l NS + NS - 1 (NS = 1, 2, 4 or 9 by S: one kernel each), alpha
// (forward) or beta (backward) in float64 registers.  The two left (right) neighbours of a lane's first (last) states arrive by
// cross-lane moves.  Per frame the wave computes the row's log-softmax once (lane c owns the classes c and c + 64, butterfly
// maximum and butterfly float64 sum: every lane ends with the same bits; trellis.h), parks it in LDS and every state gathers lp[l'_s] from
// there; the logits are loaded a frame ahead.  The forward sweep stores the alpha rows to the workspace; the backward sweep
// reads them back a frame ahead (a lane reads the cells it wrote itself), keeps beta in registers, recomputes the row's
// log-softmax and writes each gradient row once.
// occ_t[c] is summed in increasing s from a per-class list of states built once per utterance in LDS (every label occurrence
// goes into its class's list; the blank's list is the even states and is not stored).  No floating-point atomic anywhere.
//
// Arithmetic: the header's expressions as written (the pragma below and -ffp-contract=off).
#pragma clang fp contract(off)

#include <math.h>

#include "common.h"
#include "trellis.h"

#include "../../include/fhvae_ctc.h"

namespace fh {

constexpr int kCtcMaxS = 2 * FHVAE_CTC_MAX_LABELS + 1;  // 513
constexpr int kCtcCP = FHVAE_CTC_MAX_CLASSES;
constexpr int kCtcPostL = 264;  // where the labels' half of CtcLds::post begins (the blanks' half holds at most 257)
constexpr int kCtcLP = kCtcCP + 2;  // a half of the log-softmax buffer

static_assert(FHVAE_CTC_MAX_CLASSES == kTrMaxClasses && FHVAE_CTC_MAX_LABELS == kTrMaxLabels, "the lane layout of trellis.h");
static_assert(kCtcMaxS <= 64 * 9, "a lane owns at most nine states");
static_assert(kCtcPostL >= FHVAE_CTC_MAX_LABELS + 1 && kCtcPostL + FHVAE_CTC_MAX_LABELS <= kCtcMaxS + 7, "the two halves of post");

// the row's log-softmax into out[0 .. C)
__device__ __forceinline__ void ctc_log_softmax(float z0, float z1, int C, int lane, double* out) {
  const TrLogSoftmax r = tr_log_softmax(z0, z1);
  if (lane < C) out[lane] = r.l0;
  if (lane + 64 < C) out[lane + 64] = r.l1;
}

struct CtcLds {
  double lp[2 * kCtcLP];      // the log-softmax of two frames; entry kCtcCP of each half is -inf, read by states past the end
  double post[kCtcMaxS + 7];  // the last alpha row, then exp(alpha + beta - ll) of a frame in two halves
  int lab[FHVAE_CTC_MAX_LABELS];
  int cstart[kCtcCP + 1];     // the labels of class c, increasing: clist[cstart[c] .. cstart[c + 1]) (label i is state 2 i + 1)
  unsigned short clist[FHVAE_CTC_MAX_LABELS];
};

// the forward sweep, ll, and (with g) the backward sweep of one utterance of T >= 1 frames; returns ll in every lane
template <int NS>
__device__ __forceinline__ double ctc_sweeps(CtcLds& sm, const float* __restrict__ z, int64_t ldz, int T, int C, int blank, int L,
                                             double* __restrict__ arow, float* __restrict__ g, int64_t ldg, int lane) {
  const int S = 2 * L + 1;
  // cls, pen: trellis.h; a state past the end reads the -inf entry of lp, so its alpha and beta are -inf with no test in the
  // loops.  nv: the lane's states that exist
  int cls[NS];
  double pen[NS];
  const int nv = S - lane * NS;
  tr_state_classes<NS>(sm.lab, lane, S, true, blank, kCtcCP, cls, pen);
  if (lane == 0) sm.lp[kCtcCP] = -INFINITY, sm.lp[kCtcLP + kCtcCP] = -INFINITY;
#define CTC_VAL(k) ((k) < nv)
  // ---- forward
  double a[NS];
  float z0, z1, n0 = 0.f, n1 = 0.f;
  tr_load_row(z, C, lane, z0, z1);
  if (T > 1) tr_load_row(z + ldz, C, lane, n0, n1);
  ctc_log_softmax(z0, z1, C, lane, sm.lp);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = lane * NS + k;
    a[k] = s < 2 ? sm.lp[cls[k]] : -INFINITY;
    if (arow != nullptr && CTC_VAL(k)) arow[s] = a[k];
  }
  for (int t = 1; t < T; ++t) {
    z0 = n0, z1 = n1;
    if (t + 1 < T) tr_load_row(z + (int64_t)(t + 1) * ldz, C, lane, n0, n1);  // the next frame's row flies under this frame
    double* lp = sm.lp + (t & 1) * kCtcLP;
    ctc_log_softmax(z0, z1, C, lane, lp);
    __syncthreads();  // (the frame before read the other half of lp)
    double up1, up2;
    tr_left<NS>(a, lane, up1, up2);
    double b[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const double p1 = k >= 1 ? a[k >= 1 ? k - 1 : 0] : up1;
      const double p2 = k >= 2 ? a[k >= 2 ? k - 2 : 0] : (k == 1 ? up1 : up2);
      b[k] = tr_lse3(a[k], p1, p2 + pen[k]) + lp[cls[k]];
    }
    double* row = arow != nullptr ? arow + (int64_t)t * S : nullptr;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      a[k] = b[k];
      if (row != nullptr && CTC_VAL(k)) row[lane * NS + k] = a[k];
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NS; ++k)
    if (CTC_VAL(k)) sm.post[lane * NS + k] = a[k];
  __syncthreads();
  const double ll = tr_lse2(sm.post[S - 1], S >= 2 ? sm.post[S - 2] : -INFINITY);
  __syncthreads();
  if (g == nullptr || arow == nullptr || ll == -INFINITY) return ll;

  // ---- backward: beta in registers; a = alpha_t, an = alpha_{t-1} read a frame ahead
  double beta[NS], an[NS];
  double* postb = sm.post;
  double* postl = sm.post + kCtcPostL;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = lane * NS + k;
    beta[k] = (CTC_VAL(k) && s >= S - 2) ? 0.0 : -INFINITY;
    an[k] = 0.0;
  }
  tr_load_row(z + (int64_t)(T - 1) * ldz, C, lane, n0, n1);
  for (int t = T - 1; t >= 0; --t) {
    z0 = n0, z1 = n1;
    if (t > 0) {
      tr_load_row(z + (int64_t)(t - 1) * ldz, C, lane, n0, n1);
      const double* prow = arow + (int64_t)(t - 1) * S;
#pragma unroll
      for (int k = 0; k < NS; ++k) an[k] = CTC_VAL(k) ? prow[lane * NS + k] : -INFINITY;
    }
    double* lp = sm.lp + (t & 1) * kCtcLP;
    ctc_log_softmax(z0, z1, C, lane, lp);
    // exp(alpha + beta - ll), the blanks' (even states) and the labels' (odd states) side by side: postb[s / 2], postl[(s - 1) / 2]
#pragma unroll
    for (int k = 0; k < NS; ++k)
      if (CTC_VAL(k)) {
        const int s = lane * NS + k;
        ((s & 1) ? postl : postb)[s >> 1] = exp(a[k] + beta[k] - ll);
      }
    __syncthreads();
    // the gradient row: lane c sums the states of the classes c and c + 64 in increasing s
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = lane + 64 * h;
      if (c < C) {
        double occ = 0.0;
        if (c == blank) {  // L + 1 dependent additions in increasing s; the loads go eight at a time
          int i = 0;
          for (; i + 8 <= L + 1; i += 8) {
            double v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = postb[i + j];
#pragma unroll
            for (int j = 0; j < 8; ++j) occ = occ + v[j];
          }
          for (; i <= L; ++i) occ = occ + postb[i];
        } else {
          const int i0 = sm.cstart[c], i1 = sm.cstart[c + 1];
          for (int i = i0; i < i1; ++i) {
            const int li = sm.clist[i];
            occ = occ + postl[li < L ? li : 0];
          }
        }
        g[(int64_t)t * ldg + c] = (float)(exp(lp[c]) - occ);
      }
    }
    // beta_{t-1} from beta_t: gk = beta_t(s) + lp_t[l'_s]; gs = the same where the skip into s is allowed
    double gk[NS], gs[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      gk[k] = beta[k] + lp[cls[k]];
      gs[k] = gk[k] + pen[k];
    }
    double dn1 = __shfl_down(gk[0], 1, 64);                                             // state (lane + 1) NS
    double ds0 = __shfl_down(gs[0], 1, 64);                                             // state (lane + 1) NS, skip only
    double ds1 = NS >= 2 ? __shfl_down(gs[NS >= 2 ? 1 : 0], 1, 64) : __shfl_down(gs[0], 2, 64);  // state (lane + 1) NS + 1
    if (lane > 62) dn1 = -INFINITY, ds0 = -INFINITY;
    if (lane > (NS >= 2 ? 62 : 61)) ds1 = -INFINITY;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const double q1 = k + 1 < NS ? gk[k + 1 < NS ? k + 1 : 0] : dn1;
      const double q2 = k + 2 < NS ? gs[k + 2 < NS ? k + 2 : 0] : (k + 2 == NS ? ds0 : ds1);
      beta[k] = tr_lse3(gk[k], q1, q2);
      a[k] = an[k];
    }
    __syncthreads();  // post and this half of lp are free again
  }
  return ll;
#undef CTC_VAL
}

// NS: the states a lane owns.  The call launches the kernel once per NS and a workgroup whose utterance belongs to another NS
// returns at once: four lean kernels instead of one that carries the registers of all four sweeps.
template <int NS>
__global__ void __launch_bounds__(64)
    ctc_loss_kernel(const float* __restrict__ logits, int64_t ldz, int64_t n_frames, int C, int blank, const int64_t* __restrict__ utt_ptr,
                    const int32_t* __restrict__ labels, const int64_t* __restrict__ lab_ptr, const int64_t* __restrict__ cell_ptr,
                    int64_t U, double* __restrict__ nll, float* __restrict__ grad, int64_t ldg, int32_t* status, double* ws,
                    int64_t ws_cells) {
  __shared__ CtcLds sm;
  if (*status & FHVAE_CTC_BAD_PTR) return;  // (set by the check kernel)
  const int lane = threadIdx.x;
  // ---- the utterance.  Everything up to the first barrier is the same in all lanes: they return together or not at all
  const int64_t u = blockIdx.x;
  if (u >= U || C < 2 || C > kCtcCP || blank < 0 || blank >= C) return;
  const int64_t u0 = utt_ptr[u], u1 = utt_ptr[u + 1], l0 = lab_ptr[u], l1 = lab_ptr[u + 1];
  if (!tr_utt_ok(u0, u1, n_frames) || l0 < 0 || l1 < l0) return;
  const int T = (int)(u1 - u0);
  const int64_t L64 = l1 - l0;
  if (tr_states_per_lane(L64, tr_num_states(L64, true)) != NS) return;
  float* g = grad != nullptr ? grad + u0 * ldg : nullptr;
  int bits = 0;
  int L = 0;
  if (L64 > FHVAE_CTC_MAX_LABELS) {
    bits = FHVAE_CTC_BAD_LABEL;
  } else {
    L = (int)L64;
    if (tr_load_labels(labels, l0, L, C, blank, lane, sm.lab)) bits = FHVAE_CTC_BAD_LABEL;
  }
  const int S = 2 * L + 1;
  double* arow = nullptr;
  if (bits == 0 && g != nullptr && ws != nullptr && cell_ptr != nullptr) {
    const int64_t c0 = cell_ptr[u];
    if (!tr_cells_fit(c0, T, S, ws_cells)) return;  // (the check kernel has refused this already)
    arow = ws + c0;
  }
  double ll = -INFINITY;
  if (bits == 0 && T == 0) {
    if (L == 0) ll = 0.0;
  } else if (bits == 0) {
    __syncthreads();
    if (arow != nullptr) {  // the per-class lists: lane c counts, then places, the occurrences of the classes c and c + 64
      int cnt[2] = {0, 0};
      for (int i = 0; i < L; ++i) {
        const int v = sm.lab[i];
        cnt[0] += v == lane, cnt[1] += v == lane + 64;
      }
      sm.cstart[lane] = cnt[0], sm.cstart[lane + 64] = cnt[1];
      __syncthreads();
      if (lane == 0) {
        int run = 0;
        for (int c = 0; c < kCtcCP; ++c) {
          const int n = sm.cstart[c];
          sm.cstart[c] = run, run += n;
        }
        sm.cstart[kCtcCP] = run;
      }
      __syncthreads();
      int pos[2] = {sm.cstart[lane], sm.cstart[lane + 64]};
      for (int i = 0; i < L; ++i) {
        const int v = sm.lab[i];
        if (v == lane && pos[0] < FHVAE_CTC_MAX_LABELS) sm.clist[pos[0]++] = (unsigned short)i;
        if (v == lane + 64 && pos[1] < FHVAE_CTC_MAX_LABELS) sm.clist[pos[1]++] = (unsigned short)i;
      }
      __syncthreads();
    }
    const float* z = logits + u0 * ldz;
    ll = ctc_sweeps<NS>(sm, z, ldz, T, C, blank, L, arow, g, ldg, lane);
  }
  if (bits == 0 && ll == -INFINITY) bits = FHVAE_CTC_INFEASIBLE;
  if (bits != 0) {  // no likelihood: +inf and zero rows
    if (g != nullptr)
      for (int64_t i = lane; i < (int64_t)T * C; i += 64) g[(i / C) * ldg + i % C] = 0.f;
    if (lane == 0) nll[u] = INFINITY, atomicOr(status, bits);
  } else if (lane == 0) {
    nll[u] = -ll;
  }
}

static inline int64_t ctc_ws(int64_t cells) { return (cells * 8 + 255) / 256 * 256; }

}  // namespace fh

using namespace fh;

extern "C" int64_t fhvae_ctc_ws_bytes(int64_t cells) {
  if (cells < 0 || cells > (1LL << 59)) return 0;
  return ctc_ws(cells);
}

extern "C" int fhvae_ctc_loss(const float* logits, int64_t ldz, int64_t n_frames, int64_t C, int64_t blank, const int64_t* utt_ptr,
                              const int32_t* labels, const int64_t* lab_ptr, const int64_t* cell_ptr, int64_t U, double* nll,
                              float* grad, int64_t ldg, int32_t* status, void* ws, int64_t ws_bytes, void* stream) {
  FH_CHECK_PTR(status);
  if (C < 2 || blank < 0 || blank >= C || n_frames < 0 || U < 0 || ldz < C) return FHVAE_ERR_SHAPE;
  if (grad != nullptr && (ldg < C || ws_bytes < 0)) return FHVAE_ERR_SHAPE;
  if (C > FHVAE_CTC_MAX_CLASSES || n_frames > (1LL << 52)) return FHVAE_ERR_LIMIT;
  FH_CHECK_I32(U);
  if (U == 0) return FHVAE_OK;
  FH_CHECK_PTR(logits);
  FH_CHECK_PTR(utt_ptr);
  FH_CHECK_PTR(labels);
  FH_CHECK_PTR(lab_ptr);
  FH_CHECK_PTR(nll);
  if (grad != nullptr) {
    FH_CHECK_PTR(cell_ptr);
    FH_CHECK_PTR(ws);
  }
  if (ldz % 4 != 0 || ((uintptr_t)logits & 15) != 0) return FHVAE_ERR_ALIGN;
  if (((uintptr_t)utt_ptr & 7) != 0 || ((uintptr_t)labels & 3) != 0 || ((uintptr_t)lab_ptr & 7) != 0 || ((uintptr_t)nll & 7) != 0 ||
      ((uintptr_t)status & 3) != 0)
    return FHVAE_ERR_ALIGN;
  if (grad != nullptr && (ldg % 4 != 0 || ((uintptr_t)grad & 15) != 0 || ((uintptr_t)cell_ptr & 7) != 0 || ((uintptr_t)ws & 15) != 0))
    return FHVAE_ERR_ALIGN;
  if (grad == nullptr) cell_ptr = nullptr, ws = nullptr, ws_bytes = 0, ldg = 0;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tr_label_check_kernel<FHVAE_CTC_BAD_PTR>, dim3((unsigned)fh_cdiv(U, 256)), dim3(256), 0, st, utt_ptr, lab_ptr,
                     cell_ptr, U, n_frames, true, ws_bytes / 8, status);
#define CTC_LAUNCH(NS)                                                                                                          \
  hipLaunchKernelGGL(ctc_loss_kernel<NS>, dim3((unsigned)U), dim3(64), 0, st, logits, ldz, n_frames, (int)C, (int)blank, utt_ptr, \
                     labels, lab_ptr, cell_ptr, U, nll, grad, ldg, status, (double*)ws, ws_bytes / 8)
  CTC_LAUNCH(1);
  CTC_LAUNCH(2);
  CTC_LAUNCH(4);
  CTC_LAUNCH(9);
#undef CTC_LAUNCH
  return fh_launch_status();
}
