// abx.hip -- the DTW distance between every two tokens of a group, for many groups per call (include/fhvae_abx.h):
//   fhvae_abx_dtw : the hot path of the ABX phone-discrimination measure.
//
// One wavefront (a workgroup of 64 threads) per pair.  The flat pair index is the block index: a binary search in pair_ptr
// gives the group, a second one over j (j - 1) / 2 the pair (i, j), i < j, inside it -- integer comparisons only.  Then, with
// token a of n rows and token b of m rows:
//   0. lane r computes the norm of row r of a and of row r of b (float64, increasing k) into LDS;
//   1. dots: lane i owns row i of a.  The feature axis is walked in chunks of kAbxKc: the chunk of b is staged in LDS as
//      float64 (zeros past m and past D, which add nothing), the lane's chunk of its own row sits in registers, and LMAX
//      float64 accumulators (one per row of b, in registers: the j loop is unrolled and guarded per 8 rows by the
//      wave-uniform m) take one fused multiply-add per k, in increasing k.  Every b value is an LDS broadcast;
//   2. costs: the n x m cells are spread flat over the lanes (a short token does not idle the wave through the division and
//      the acos), read as float64 dots from LDS and written back as f32 costs IN PLACE: cell y's cost occupies the low half
//      of float64 cell y / 2, which the round that reads cell y has already consumed (one barrier per round covers round 0);
//   3. the DTW recursion as an anti-diagonal sweep: at step t lane i computes cell (i, t - i) from its own last value (left),
//      lane i - 1's last value (up, one shuffle) and the one before that (diagonal, kept from the previous step).
// A row of the cost image is n rounded up to even, so the sweep's lane stride (row - 1) is odd: no LDS bank conflict.
// The caller's bound on the token length picks the instance (LMAX = 16, 32 or 64 rows per token).
//
// Arithmetic: exactly the header's.  No contraction (the pragma below and -ffp-contract=off), correctly rounded f32 division;
// the fused multiply-adds are explicit and exact-product, so they equal the unfused float64 sums.  No atomics except the
// atomicOr of the status word.
#pragma clang fp contract(off)

#include <math.h>

#include "common.h"

#include "abx_cost.h"

namespace fh {

constexpr int kAbxLanes = 64;  // one wavefront per pair; lane i owns row i of token a
constexpr int kAbxKc = 8;      // features per staged chunk of token b
constexpr int kAbxBad = FHVAE_ABX_BAD_TOKEN | FHVAE_ABX_BAD_PTR;

static_assert(FHVAE_ABX_MAX_LEN == kAbxLanes, "a token's rows map onto the lanes of one wavefront");
static_assert(kAbxKc == 8, "the dot loop walks the rows of b in blocks of 8, as many as a chunk has features");

// the last g in [0, G) with ptr[g] <= x (0 when there is none); reads ptr[0 .. G - 1] only
__device__ __forceinline__ int64_t abx_find(const int64_t* __restrict__ ptr, int64_t G, int64_t x) {
  int64_t lo = 0, hi = G - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (ptr[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ bool abx_token_ok(int64_t start, int len, int max_len, int64_t n_frames) {
  return len >= 1 && len <= max_len && start >= 0 && start <= n_frames - len;
}

// one thread per token and per group: the rules of the header
__global__ void abx_check_kernel(const int64_t* __restrict__ tok_start, const int32_t* __restrict__ tok_len, int64_t N, int max_len,
                                 int64_t n_frames, const int64_t* __restrict__ grp_ptr, const int64_t* __restrict__ out_ptr,
                                 const int64_t* __restrict__ pair_ptr, int64_t G, int64_t n_pairs, int64_t n_out, int32_t* status) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < N && !abx_token_ok(tok_start[t], tok_len[t], max_len, n_frames)) atomicOr(status, FHVAE_ABX_BAD_TOKEN);
  if (t < G) {
    const int64_t a = grp_ptr[t], b = grp_ptr[t + 1], o0 = out_ptr[t], o1 = out_ptr[t + 1], p0 = pair_ptr[t], p1 = pair_ptr[t + 1];
    // (ranges before differences and products: n <= N < 2^31, so n * n does not overflow)
    bool ok = a >= 0 && b >= a && b <= N && o0 >= 0 && o1 >= o0 && o1 <= n_out && p0 >= 0 && p1 >= p0 && p1 <= n_pairs;
    if (ok) {
      const int64_t n = b - a;
      ok = o1 - o0 == n * n && p1 - p0 == n * (n - 1) / 2;
    }
    if (t == 0) ok = ok && a == 0 && o0 == 0 && p0 == 0;
    if (t == G - 1) ok = ok && b == N && o1 == n_out && p1 == n_pairs;
    if (!ok) atomicOr(status, FHVAE_ABX_BAD_PTR);
  }
}

// one thread per token: the zero of its group's diagonal
__global__ void abx_diag_kernel(const int64_t* __restrict__ grp_ptr, const int64_t* __restrict__ out_ptr, int64_t G, int64_t N,
                                int64_t n_out, float* __restrict__ out, const int32_t* status) {
  if (*status & kAbxBad) return;  // (set by the check kernel)
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N) return;
  const int64_t g = abx_find(grp_ptr, G, t);
  const int64_t a = grp_ptr[g], b = grp_ptr[g + 1], o = out_ptr[g];
  if (!(a >= 0 && a <= t && t < b && b <= N && o >= 0)) return;
  const int64_t n = b - a, k = t - a;
  if (o > n_out - n * n) return;
  out[o + k * n + k] = 0.f;
}

// LMAX: the rows a token may have in this instance (16, 32 or 64): it sizes the LDS images and the accumulators, and with them
// the wavefronts a CU holds: one per SIMD at 64 rows (37 KB of LDS each), two at 16 and 32 rows, where the registers bind (the
// scheduler hoists the LDS reads of a chunk above its multiply-adds and takes 208 / 240 of them; held to 128 or 168 by
// __launch_bounds__, or fenced with sched_barrier, the same code spills 66 to 106 registers into the loop).  The arithmetic of a
// pair does not depend on LMAX
template <int LMAX>
__global__ void __launch_bounds__(kAbxLanes, LMAX <= 32 ? 2 : 1) abx_dtw_kernel(const float* __restrict__ feats, int64_t n_frames, int D,
                                                            const int64_t* __restrict__ tok_start,
                                                            const int32_t* __restrict__ tok_len, int64_t N,
                                                            const int64_t* __restrict__ grp_ptr, const int64_t* __restrict__ out_ptr,
                                                            const int64_t* __restrict__ pair_ptr, int64_t G, int64_t n_pairs,
                                                            int64_t n_out, int metric, float* __restrict__ out,
                                                            const int32_t* status) {
  __shared__ double dots[LMAX * LMAX];  // (j, i) at j * ns + i: float64 dots, then (in place) the f32 costs
  __shared__ double bs[LMAX * kAbxKc];  // the staged chunk of token b: (j, kk) at j * kAbxKc + kk
  __shared__ double nrm[2 * LMAX];      // the row norms of a, then those of b
  if (*status & kAbxBad) return;  // (set by the check kernel)
  const int lane = threadIdx.x;
  // ---- the pair.  Everything up to the first barrier is the same in all lanes: they return together or not at all
  const int64_t p = blockIdx.x;
  if (p >= n_pairs) return;
  const int64_t g = abx_find(pair_ptr, G, p);
  const int64_t g0 = grp_ptr[g], g1 = grp_ptr[g + 1], ob = out_ptr[g];
  if (!(g0 >= 0 && g1 > g0 && g1 <= N)) return;
  const int64_t ng = g1 - g0, q = p - pair_ptr[g];
  if (q < 0 || q >= ng * (ng - 1) / 2 || ob < 0 || ob > n_out - ng * ng) return;
  int64_t lo = 1, hi = ng - 1;  // the last tj in [1, ng) with tj (tj - 1) / 2 <= q
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (mid * (mid - 1) / 2 <= q) lo = mid; else hi = mid - 1;
  }
  const int64_t tj = lo, ti = q - tj * (tj - 1) / 2;  // ti < tj
  if (ti >= tj) return;
  const int64_t sa = tok_start[g0 + ti], sb = tok_start[g0 + tj];
  const int n = tok_len[g0 + ti], m = tok_len[g0 + tj];
  if (!abx_token_ok(sa, n, LMAX, n_frames) || !abx_token_ok(sb, m, LMAX, n_frames)) return;
  const int ns = (n + 1) & ~1;  // a row of the dot / cost image

  // ---- 0. norms
  if (lane < n) {
    const float* r = feats + (sa + lane) * D;
    double s = 0.0;
    for (int k = 0; k < D; ++k) {
      const double x = (double)r[k];
      s = __builtin_fma(x, x, s);
    }
    nrm[lane] = sqrt(s);
  }
  if (lane < m) {
    const float* r = feats + (sb + lane) * D;
    double s = 0.0;
    for (int k = 0; k < D; ++k) {
      const double x = (double)r[k];
      s = __builtin_fma(x, x, s);
    }
    nrm[LMAX + lane] = sqrt(s);
  }

  // ---- 1. dots
  double acc[LMAX];
#pragma unroll
  for (int j = 0; j < LMAX; ++j) acc[j] = 0.0;
  const float* ra = feats + (sa + (lane < n ? lane : n - 1)) * D;  // (a lane without a row reads the last one; its sums are unused)
  for (int k0 = 0; k0 < D; k0 += kAbxKc) {
    __syncthreads();  // the chunk before is consumed
    for (int idx = lane; idx < LMAX * kAbxKc; idx += kAbxLanes) {
      const int j = idx / kAbxKc, k = k0 + idx % kAbxKc;
      bs[idx] = (j < m && k < D) ? (double)feats[(sb + j) * D + k] : 0.0;
    }
    double av[kAbxKc];
#pragma unroll
    for (int kk = 0; kk < kAbxKc; ++kk) av[kk] = k0 + kk < D ? (double)ra[k0 + kk] : 0.0;
    __syncthreads();
#pragma unroll
    for (int j0 = 0; j0 < LMAX; j0 += 8) {
      if (j0 < m) {
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
#pragma unroll
          for (int kk = 0; kk < kAbxKc; ++kk) acc[j0 + jj] = __builtin_fma(av[kk], bs[(j0 + jj) * kAbxKc + kk], acc[j0 + jj]);
        }
      }
    }
  }
  if (lane < n) {
#pragma unroll
    for (int j = 0; j < LMAX; ++j) {
      if (j < m) dots[j * ns + lane] = acc[j];
    }
  }
  __syncthreads();

  // ---- 2. costs, in place
  float* cost = (float*)dots;
  const int total = ns * m;
  for (int base = 0; base < total; base += kAbxLanes) {
    const int y = base + lane, j = y / ns, i = y - j * ns;
    const bool act = y < total && i < n;
    double c = 0.0;
    if (act) c = abx_frame_cost(dots[y], nrm[i], nrm[LMAX + j], metric);
    __syncthreads();  // every dot of this round is read before a cost lands on one (round 0; later rounds write behind)
    if (act) cost[y] = (float)c;
  }
  __syncthreads();

  // ---- 3. the sweep
  float myD = 0.f, diagD = 0.f;
  int myL = 0, diagL = 0;
  for (int t = 0; t < n + m - 1; ++t) {
    const float upD = __shfl_up(myD, 1, 64);  // D[i - 1][t - i]: lane i - 1 after step t - 1
    const int upL = __shfl_up(myL, 1, 64);
    const int j = t - lane;
    if (lane < n && j >= 0 && j < m) {
      const float c = cost[j * ns + lane];
      float pd = 0.f;  // (cell (0, 0): 0 + c = c exactly)
      int pl = 0;
      if (lane == 0) {
        if (j > 0) pd = myD, pl = myL;
      } else if (j == 0) {
        pd = upD, pl = upL;
      } else {
        pd = diagD, pl = diagL;
        if (upD < pd) pd = upD, pl = upL;
        if (myD < pd) pd = myD, pl = myL;
      }
      myD = pd + c;
      myL = pl + 1;
    }
    diagD = upD, diagL = upL;
  }
  if (lane == n - 1) {
    const float d = myD / (float)myL;
    out[ob + ti * ng + tj] = d;
    out[ob + tj * ng + ti] = d;
  }
}

}  // namespace fh

using namespace fh;

extern "C" int fhvae_abx_dtw(const float* feats, int64_t n_frames, int64_t D, const int64_t* tok_start, const int32_t* tok_len,
                             int64_t N, int64_t max_len, const int64_t* grp_ptr, const int64_t* out_ptr, const int64_t* pair_ptr, int64_t G,
                             int64_t n_pairs, int64_t n_out, int metric, float* out, int32_t* status, void* stream) {
  FH_CHECK_PTR(status);
  if (metric != FHVAE_ABX_ANGULAR && metric != FHVAE_ABX_COSINE) return FHVAE_ERR_SHAPE;
  if (D < 1 || N < 0 || G < 0 || n_frames < 0 || n_pairs < 0 || n_out < 0) return FHVAE_ERR_SHAPE;
  if (max_len < 1) return FHVAE_ERR_SHAPE;
  if (D > FHVAE_ABX_MAX_DIM || max_len > FHVAE_ABX_MAX_LEN) return FHVAE_ERR_LIMIT;
  FH_CHECK_I32(N);
  FH_CHECK_I32(G);
  FH_CHECK_I32(n_pairs);  // (one workgroup per pair)
  if (N == 0 || G == 0) return FHVAE_OK;
  FH_CHECK_PTR(feats);
  FH_CHECK_PTR(tok_start);
  FH_CHECK_PTR(tok_len);
  FH_CHECK_PTR(grp_ptr);
  FH_CHECK_PTR(out_ptr);
  FH_CHECK_PTR(pair_ptr);
  if (n_out > 0) FH_CHECK_PTR(out);
  hipStream_t st = (hipStream_t)stream;
  const int64_t cblocks = fh_cdiv(N > G ? N : G, 256), dblocks = fh_cdiv(N, 256);
  hipLaunchKernelGGL(abx_check_kernel, dim3((unsigned)cblocks), dim3(256), 0, st, tok_start, tok_len, N, (int)max_len, n_frames, grp_ptr,
                     out_ptr, pair_ptr, G, n_pairs, n_out, status);
  hipLaunchKernelGGL(abx_diag_kernel, dim3((unsigned)dblocks), dim3(256), 0, st, grp_ptr, out_ptr, G, N, n_out, out, status);
  if (n_pairs > 0)
    hipLaunchKernelGGL(max_len <= 16 ? abx_dtw_kernel<16> : (max_len <= 32 ? abx_dtw_kernel<32> : abx_dtw_kernel<64>), dim3((unsigned)n_pairs), dim3(kAbxLanes), 0, st, feats, n_frames, (int)D, tok_start, tok_len, N,
                       grp_ptr, out_ptr, pair_ptr, G, n_pairs, n_out, metric, out, status);
  return fh_launch_status();
}
