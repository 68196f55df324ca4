// qbe.hip -- subsequence DTW of every query against every utterance (include/fhvae_qbe.h):
//   fhvae_qbe_sdtw : the hot path of query-by-example search.
//
// One wavefront (a workgroup of 64 threads) per (query, utterance) cell; the block index is u * Q + q, so the workgroups in
// flight together read the same utterance.  The utterance is walked in column tiles of kQbeW = 64 frames.  With a query of n
// rows, per tile:
//   1. dots: lane l owns column l of the tile (its frame sits in registers, chunk by chunk of kQbeKc features), the chunk of
//      the query is staged in LDS as float64 (zeros past n and past D, which add nothing) and LMAX float64 accumulators (one
//      per query row, in registers: the row loop is unrolled and guarded per 8 rows by the wave-uniform n) take one fused
//      multiply-add per k, in increasing k.  Every query value is an LDS broadcast.  The lane's own norm is summed beside them;
//      the query's norms are computed once per cell.  With one or two wavefronts per SIMD nothing else hides a load, so the
//      next chunk's global loads are issued before this chunk's multiply-adds (8 to 19 % of the call's time, measured);
//   2. costs: the lane turns its n dots into f32 costs (abx_cost.h) and writes them into the cost ring in LDS: the ring holds
//      two tiles, (i, j) at i * 2 kQbeW + j mod 2 kQbeW.  No image of float64 dots is kept in LDS;
//   3. the recursion as one anti-diagonal sweep over the whole utterance, as abx.hip's: at step t lane i computes cell
//      (i, t - i) from its own last value (left), lane i - 1's last value (up, one shuffle) and the one before that (diagonal,
//      kept from the previous step).  The sweep does not restart at a tile: steps 64 k .. 64 k + 63 run once tile k is in the
//      ring, and they touch columns 64 k - 63 .. 64 k + 63 only, tiles k - 1 and k, so a lane's last (D, L, S) and its diagonal
//      simply stay in its registers across the tile boundary, and every step but the first n - 1 and the last n - 1 of the
//      utterance has all n lanes at work.  At step t the lanes' columns t - i are distinct mod 64: no LDS bank conflict.
// Lane n - 1 finishes one column per step: it keeps the best (strictly smaller, so the smallest j wins) and, when a profile
// is asked for, parks e and s in LDS; after every 64 steps the wave writes the 64 columns finished in them side by side.
// The caller's bound on the query length picks the instance (LMAX = 16, 32 or 64 rows).
//
// Arithmetic: exactly the header's.  No contraction (the pragma below and -ffp-contract=off), correctly rounded f32 division;
// the fused multiply-adds are explicit and exact-product, so they equal the unfused float64 sums.  No atomics except the
// atomicOr of the status word.
#pragma clang fp contract(off)

#include <math.h>

#include "common.h"

#include "abx_cost.h"

#include "../../include/fhvae_qbe.h"

namespace fh {

constexpr int kQbeLanes = 64;  // one wavefront per cell; lane i owns query row i in the sweep and column i of a tile in the dots
constexpr int kQbeW = 64;      // columns per tile
constexpr int kQbeRing = 2 * kQbeW;  // columns of the cost ring
constexpr int kQbeKc = 8;      // features per staged chunk of the query
constexpr int kQbeBad = FHVAE_QBE_BAD_QUERY | FHVAE_QBE_BAD_PTR;

static_assert(FHVAE_QBE_MAX_QLEN == kQbeLanes, "a query's rows map onto the lanes of one wavefront");
static_assert(kQbeW == kQbeLanes, "a tile's columns map onto the lanes of one wavefront");
static_assert(FHVAE_QBE_ANGULAR == FHVAE_ABX_ANGULAR && FHVAE_QBE_COSINE == FHVAE_ABX_COSINE, "abx_frame_cost takes the metric");
static_assert(FHVAE_QBE_MAX_DIM == FHVAE_ABX_MAX_DIM, "the frame cost is ABX's");

__device__ __forceinline__ bool qbe_query_ok(int64_t start, int len, int max_len, int64_t nq_frames) {
  return len >= 1 && len <= max_len && start >= 0 && start <= nq_frames - len;
}

__device__ __forceinline__ bool qbe_utt_ok(int64_t a, int64_t b, int64_t n_frames) {
  return a >= 0 && b >= a && b <= n_frames && b - a <= 0x7fffffffLL;
}

// one thread per query and per utterance: the rules of the header
__global__ void qbe_check_kernel(const int64_t* __restrict__ q_start, const int32_t* __restrict__ q_len, int64_t Q, int max_qlen,
                                 int64_t nq_frames, const int64_t* __restrict__ utt_ptr, int64_t U, int64_t n_frames, int32_t* status) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < Q && !qbe_query_ok(q_start[t], q_len[t], max_qlen, nq_frames)) atomicOr(status, FHVAE_QBE_BAD_QUERY);
  if (t < U) {
    const int64_t a = utt_ptr[t], b = utt_ptr[t + 1];
    bool ok = qbe_utt_ok(a, b, n_frames);
    if (t == 0) ok = ok && a == 0;
    if (t == U - 1) ok = ok && b == n_frames;
    if (!ok) atomicOr(status, FHVAE_QBE_BAD_PTR);
  }
}

// LMAX: the rows a query may have in this instance (16, 32 or 64): it sizes the cost ring (LMAX * 512 bytes) and the
// accumulators, and with them the wavefronts a CU holds: two per SIMD at 16 rows (256 registers, 7 of them spilled), one at 32
// and 64 rows (305 and 388 registers, 37 KB of LDS at 64 rows; held to 256 registers the 32-row instance spills more than 23).
// The arithmetic of a cell does not depend on LMAX
template <int LMAX>
__global__ void __launch_bounds__(kQbeLanes, LMAX <= 16 ? 2 : 1)
    qbe_sdtw_kernel(const float* __restrict__ qfeats, int64_t nq_frames, const float* __restrict__ feats, int64_t n_frames, int D,
                    const int64_t* __restrict__ q_start, const int32_t* __restrict__ q_len, int64_t Q,
                    const int64_t* __restrict__ utt_ptr, int64_t U, int metric, float* __restrict__ best_cost,
                    int32_t* __restrict__ best_start, int32_t* __restrict__ best_end, float* __restrict__ end_cost,
                    int32_t* __restrict__ end_start, const int32_t* status) {
  __shared__ float cost[LMAX * kQbeRing];  // (i, j) at i * kQbeRing + j % kQbeRing
  __shared__ double qs[kQbeLanes * kQbeKc];  // the staged chunk of the query: (i, kk) at i * kQbeKc + kk; then 8 dots per lane
  __shared__ double qn[LMAX];              // the query's row norms
  __shared__ float pe[kQbeW];              // the profile of the last 64 steps: column j at j % kQbeW
  __shared__ int ps[kQbeW];
  if (*status & kQbeBad) return;  // (set by the check kernel)
  const int lane = threadIdx.x;
  // ---- the cell.  Everything up to the first barrier is the same in all lanes: they return together or not at all
  const int64_t cell = blockIdx.x;
  if (cell >= Q * U) return;
  const int64_t u = cell / Q, q = cell - u * Q;
  const int64_t sq = q_start[q], u0 = utt_ptr[u], u1 = utt_ptr[u + 1];
  const int n = q_len[q];
  if (!qbe_query_ok(sq, n, LMAX, nq_frames) || !qbe_utt_ok(u0, u1, n_frames)) return;
  const int m = (int)(u1 - u0);
  const int64_t o = q * U + u;
  if (m == 0) {
    if (lane == 0) best_cost[o] = INFINITY, best_start[o] = -1, best_end[o] = -1;
    return;
  }
  const bool profile = end_cost != nullptr || end_start != nullptr;
  const int64_t prow = q * n_frames + u0;  // the cell's first profile column

  // ---- 0. the query's norms
  if (lane < n) {
    const float* r = qfeats + (sq + lane) * D;
    double s = 0.0;
    for (int k = 0; k < D; ++k) {
      const double x = (double)r[k];
      s = __builtin_fma(x, x, s);
    }
    qn[lane] = sqrt(s);
  }

  float myD = 0.f, diagD = 0.f, bestE = INFINITY;
  int myL = 0, diagL = 0, myS = 0, diagS = 0, bestS = -1, bestJ = -1;
  const int64_t steps = (int64_t)n + m - 1;  // (m may be 2^31 - 1: the steps count in int64)
  for (int64_t t0 = 0; t0 < steps; t0 += kQbeW) {
    if (t0 < m) {
      // ---- 1. the dots of tile t0 / 64: lane = column
      const bool have = t0 + lane < m;
      const int j = have ? (int)t0 + lane : m - 1;  // (a lane without a column reads the last one; its sums are unused)
      const float* rb = feats + (u0 + j) * D;
      double acc[LMAX];
#pragma unroll
      for (int i = 0; i < LMAX; ++i) acc[i] = 0.0;
      double nb2 = 0.0;
      // a chunk travels as f32 in registers: the lane's own 8 features and its share of the query's chunk
      constexpr int kQr = LMAX * kQbeKc / kQbeLanes;
      float braw[kQbeKc], qraw[kQr];
      auto load_chunk = [&](int k0) {
#pragma unroll
        for (int kk = 0; kk < kQbeKc; ++kk) braw[kk] = k0 + kk < D ? rb[k0 + kk] : 0.f;
#pragma unroll
        for (int r = 0; r < kQr; ++r) {
          const int idx = lane + r * kQbeLanes, i = idx / kQbeKc, k = k0 + idx % kQbeKc;
          qraw[r] = (i < n && k < D) ? qfeats[(sq + i) * D + k] : 0.f;
        }
      };
      load_chunk(0);
      for (int k0 = 0; k0 < D; k0 += kQbeKc) {
        __syncthreads();  // the chunk before is consumed (and, first, the sweep before has read what this tile replaces)
#pragma unroll
        for (int r = 0; r < kQr; ++r) qs[lane + r * kQbeLanes] = (double)qraw[r];
        double bv[kQbeKc];
#pragma unroll
        for (int kk = 0; kk < kQbeKc; ++kk) {
          bv[kk] = (double)braw[kk];
          nb2 = __builtin_fma(bv[kk], bv[kk], nb2);
        }
        if (k0 + kQbeKc < D) load_chunk(k0 + kQbeKc);  // the next chunk's loads fly under this chunk's multiply-adds
        __syncthreads();
#pragma unroll
        for (int i0 = 0; i0 < LMAX; i0 += 8) {
          if (i0 < n) {
#pragma unroll
            for (int ii = 0; ii < 8; ++ii) {
#pragma unroll
              for (int kk = 0; kk < kQbeKc; ++kk) acc[i0 + ii] = __builtin_fma(qs[(i0 + ii) * kQbeKc + kk], bv[kk], acc[i0 + ii]);
            }
          }
        }
      }
      // ---- 2. the costs of the lane's column into the ring.  The accumulators are indexed by constants only, so 8 rows at a
      // time pass through the lane's own slots of qs and a rolled loop holds the one copy of the division and the acos
      __syncthreads();  // the query's last chunk is consumed
      const double nb = sqrt(nb2);
      const int col = j & (kQbeRing - 1);
#pragma unroll
      for (int i0 = 0; i0 < LMAX; i0 += 8) {
        if (i0 < n) {
#pragma unroll
          for (int ii = 0; ii < 8; ++ii) qs[ii * kQbeLanes + lane] = acc[i0 + ii];
          const int rows = n - i0 < 8 ? n - i0 : 8;
#pragma unroll 1
          for (int ii = 0; ii < rows; ++ii) {
            if (have) cost[(i0 + ii) * kQbeRing + col] = (float)abx_frame_cost(qs[ii * kQbeLanes + lane], qn[i0 + ii], nb, metric);
          }
        }
      }
    }
    __syncthreads();

    // ---- 3. the sweep, steps t0 .. t0 + 63
    const int64_t t1 = t0 + kQbeW < steps ? t0 + kQbeW : steps;
    for (int64_t t = t0; t < t1; ++t) {
      const float upD = __shfl_up(myD, 1, 64);  // D[i - 1][t - i]: lane i - 1 after step t - 1
      const int upL = __shfl_up(myL, 1, 64);
      const int upS = __shfl_up(myS, 1, 64);
      const int64_t j64 = t - lane;
      if (lane < n && j64 >= 0 && j64 < m) {
        const int j = (int)j64;
        const float c = cost[lane * kQbeRing + (j & (kQbeRing - 1))];
        float pd = 0.f;  // (row 0: 0 + c = c exactly)
        int pl = 0, pst = j;
        if (lane > 0) {
          if (j == 0) {
            pd = upD, pl = upL, pst = upS;
          } else {
            pd = diagD, pl = diagL, pst = diagS;
            if (upD < pd) pd = upD, pl = upL, pst = upS;
            if (myD < pd) pd = myD, pl = myL, pst = myS;
          }
        }
        myD = pd + c;
        myL = pl + 1;
        myS = pst;
        if (lane == n - 1) {
          const float e = myD / (float)myL;
          if (e < bestE) bestE = e, bestS = myS, bestJ = j;
          if (profile) pe[j & (kQbeW - 1)] = e, ps[j & (kQbeW - 1)] = myS;
        }
      }
      diagD = upD, diagL = upL, diagS = upS;
    }
    if (profile) {
      // the columns finished in these steps: t - (n - 1) for t in [t0, t1)
      __syncthreads();
      const int64_t j64 = t0 - (n - 1) + lane;
      if (j64 >= 0 && j64 < m && j64 <= t1 - 1 - (n - 1)) {
        if (end_cost) end_cost[prow + j64] = pe[j64 & (kQbeW - 1)];
        if (end_start) end_start[prow + j64] = ps[j64 & (kQbeW - 1)];
      }
      __syncthreads();
    }
  }
  if (lane == n - 1) best_cost[o] = bestE, best_start[o] = bestS, best_end[o] = bestJ;
}

}  // namespace fh

using namespace fh;

extern "C" int fhvae_qbe_sdtw(const float* qfeats, int64_t nq_frames, const float* feats, int64_t n_frames, int64_t D,
                              const int64_t* q_start, const int32_t* q_len, int64_t Q, int64_t max_qlen, const int64_t* utt_ptr, int64_t U,
                              int metric, float* best_cost, int32_t* best_start, int32_t* best_end, float* end_cost, int32_t* end_start,
                              int32_t* status, void* stream) {
  FH_CHECK_PTR(status);
  if (metric != FHVAE_QBE_ANGULAR && metric != FHVAE_QBE_COSINE) return FHVAE_ERR_SHAPE;
  if (D < 1 || Q < 0 || U < 0 || nq_frames < 0 || n_frames < 0) return FHVAE_ERR_SHAPE;
  if (max_qlen < 1) return FHVAE_ERR_SHAPE;
  if (D > FHVAE_QBE_MAX_DIM || max_qlen > FHVAE_QBE_MAX_QLEN) return FHVAE_ERR_LIMIT;
  FH_CHECK_I32(Q);
  FH_CHECK_I32(U);
  if (Q > 0 && U > 0x7fffffffLL / Q) return FHVAE_ERR_LIMIT;  // (one workgroup per cell)
  if ((end_cost || end_start) && Q > 0 && n_frames > INT64_MAX / Q) return FHVAE_ERR_LIMIT;
  if (Q == 0 || U == 0) return FHVAE_OK;
  FH_CHECK_PTR(qfeats);
  FH_CHECK_PTR(feats);
  FH_CHECK_PTR(q_start);
  FH_CHECK_PTR(q_len);
  FH_CHECK_PTR(utt_ptr);
  FH_CHECK_PTR(best_cost);
  FH_CHECK_PTR(best_start);
  FH_CHECK_PTR(best_end);
  hipStream_t st = (hipStream_t)stream;
  const int64_t cblocks = fh_cdiv(Q > U ? Q : U, 256);
  hipLaunchKernelGGL(qbe_check_kernel, dim3((unsigned)cblocks), dim3(256), 0, st, q_start, q_len, Q, (int)max_qlen, nq_frames, utt_ptr, U,
                     n_frames, status);
  hipLaunchKernelGGL(max_qlen <= 16 ? qbe_sdtw_kernel<16> : (max_qlen <= 32 ? qbe_sdtw_kernel<32> : qbe_sdtw_kernel<64>),
                     dim3((unsigned)(Q * U)), dim3(kQbeLanes), 0, st, qfeats, nq_frames, feats, n_frames, (int)D, q_start, q_len, Q, utt_ptr, U,
                     metric, best_cost, best_start, best_end, end_cost, end_start, status);
  return fh_launch_status();
}
