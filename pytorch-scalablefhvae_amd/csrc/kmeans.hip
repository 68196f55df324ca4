// kmeans.hip -- the two halves of a Lloyd iteration on (N, D) f32 rows (include/fhvae_kmeans.h):
//   fhvae_km_assign : every row's nearest centroid, and its squared distance;
//   fhvae_km_update : every centroid as the mean of its members, and every cluster's inertia.
//
// Assignment is allpairs_f32.h's pass with an arg-min epilogue.  A workgroup of 256 threads keeps 256 rows of x stationary and
// streams ALL K centroids through LDS in tiles of 64; `side` puts the tile's cn beside it (+inf past K: a padded row has dot
// 0 and score +inf, it never wins), `pair` turns a lane's four dots of a tile into scores and keeps a running (best, k) per
// stationary row.  A lane meets its k in increasing order (tile, block of 16, register), so the strict < keeps the first
// of equal scores; at the end the four lanes of a row merge by the two xor shuffles of ap::quad_min, carrying the index
// (smaller score, then smaller k: commutative, so the four agree).  No (N, K) matrix, no second pass, nothing a row's
// result could take from its neighbours.
//
// The update has no floating-point atomics.  A piece is FHVAE_KM_PIECE consecutive members of one cluster; there are at most
// N / 256 + K of them.  km_piece_prefix_kernel turns cl_ptr into the prefix of pieces per cluster; km_piece_kernel runs over the
// bound (surplus pieces return), finds its cluster by a binary search in that prefix -- integer comparisons only -- and sums
// its members per column in member order in float64, one thread per column; km_combine_kernel adds a cluster's piece sums in piece
// order per (k, d), divides and rounds once.  The grid decides nothing about the order.
//
// Arithmetic: exactly the header's.  No contraction (the pragma below and -ffp-contract=off); the fmaf of the norms and of
// the score are explicit.  No atomics except the atomicOr of the status word.
#pragma clang fp contract(off)

#include <math.h>

#include "allpairs_f32.h"

#include "../../include/fhvae_kmeans.h"

namespace fh {

namespace {

constexpr int kKmYT = ap::kYT;
constexpr int kKmBad = FHVAE_KM_BAD_PTR | FHVAE_KM_BAD_PERM;
constexpr int kKmPiece = FHVAE_KM_PIECE;
constexpr int kKmScan = 1024;  // threads of the one workgroup that builds the piece prefix

static_assert(kKmYT == 64, "side() fills one cn per streamed row of a tile with the first 64 threads");

// ---- workspace: cn (K) f32 | xn (N) f32 | piece prefix (K + 1) int64 | piece sums (pieces, D) f64 | piece inertia (pieces) f64
struct KmWs {
  int64_t cn, xn, pp, psum, pin, total, max_pieces;
};
inline int64_t km_pad(int64_t b) { return fh_cdiv(b, 256) * 256; }
inline KmWs km_ws(int64_t N, int64_t K, int64_t D) {
  KmWs w;
  w.max_pieces = fh_cdiv(N, kKmPiece) + K;
  w.cn = 0;
  w.xn = w.cn + km_pad(K * 4);
  w.pp = w.xn + km_pad(N * 4);
  w.psum = w.pp + km_pad((K + 1) * 8);
  w.pin = w.psum + km_pad(w.max_pieces * D * 8);
  w.total = w.pin + km_pad(w.max_pieces * 8);
  return w;
}

// out[r] = sum_d m[r][d]^2: one thread per row, one fma chain in d order (as sv_norm_kernel, without the square root)
__global__ void km_sqnorm_kernel(const float* __restrict__ m, int64_t ld, int64_t rows, int D, float* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const float* p = m + r * ld;
  float ss = 0.f;
  for (int d = 0; d < D; d += 4) {
    const float4 v = *(const float4*)(p + d);
    ss = __builtin_fmaf(v.x, v.x, ss);
    ss = __builtin_fmaf(v.y, v.y, ss);
    ss = __builtin_fmaf(v.z, v.z, ss);
    ss = __builtin_fmaf(v.w, v.w, ss);
  }
  out[r] = ss;
}

struct KmAssignArgs {
  const float* x;
  const float* cent;
  const float* cn;  // (K)
  const float* xn;  // (N); read only when dist is written
  int32_t* assign;
  float* dist;  // or nullptr
  int64_t ldx, ldc;
  int N, K;
};

// (D > 96: 128 and more registers of stationary fragments; two workgroups per CU would spill, as in sv.hip)
template <int D>
__global__ __launch_bounds__(256, D > 96 ? 1 : 2) void km_assign_kernel(KmAssignArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ytile = smem;                          // [64][D] f32, swizzled
  float* cnl = (float*)(smem + kKmYT * D * 4);  // [64]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i = lane & 15;
  const int x0 = (int)blockIdx.x * 256 + wave * 64;  // (N <= 2^30: no overflow)
  const int K = a.K;

  uint4 xf[4][D / 16];
  ap::load_stationary<D>(a.x, a.ldx, a.N, x0, xf);
  float best[4];
  int bk[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) best[t] = INFINITY, bk[t] = 0;

  ap::stream<D>(
      a.cent, a.ldc, 0, K, ytile, xf,
      [&](int y0) {
        if (tid < kKmYT) cnl[tid] = y0 + tid < K ? a.cn[y0 + tid] : INFINITY;
      },
      ap::EveryBlock(),
      [&](int y0, int yb, const f32x4(&acc)[4]) {
        const float4 cv = *(const float4*)(cnl + yb * 16 + 4 * g);
        const float cr[4] = {cv.x, cv.y, cv.z, cv.w};
        const int kb = y0 + yb * 16 + 4 * g;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float s = __builtin_fmaf(-2.f, acc[t][r], cr[r]);
            if (s < best[t]) best[t] = s, bk[t] = kb + r;
          }
        }
      });

  // ---- the four lanes of a row: smaller score, then smaller k
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float ob = __shfl_xor(best[t], o, 64);
      const int ok = __shfl_xor(bk[t], o, 64);
      if (ob < best[t] || (ob == best[t] && ok < bk[t])) best[t] = ob, bk[t] = ok;
    }
    const int row = x0 + t * 16 + i;
    if (g == 0 && row < a.N) {
      a.assign[row] = bk[t];
      if (a.dist != nullptr) a.dist[row] = fmaxf(a.xn[row] + best[t], 0.f);
    }
  }
}

template <int D>
int km_assign_launch(const KmAssignArgs& a, hipStream_t st) {
  const int smem = kKmYT * D * 4 + kKmYT * 4;
  hipLaunchKernelGGL(km_assign_kernel<D>, dim3((unsigned)fh_cdiv(a.N, 256)), dim3(256), (size_t)smem, st, a);
  return fh_launch_status();
}

// ---- update
__device__ __forceinline__ int64_t km_pieces_of(int64_t c) { return (c + kKmPiece - 1) / kKmPiece; }

// the members [a, b) of cluster k, or false if cl_ptr does not give an interval inside [0, N]
__device__ __forceinline__ bool km_cluster(const int64_t* __restrict__ cl_ptr, int64_t k, int64_t N, int64_t& a, int64_t& b) {
  a = cl_ptr[k], b = cl_ptr[k + 1];
  return a >= 0 && b >= a && b <= N;
}

// one thread per row and per cluster: the rules of the header
__global__ void km_check_kernel(const int64_t* __restrict__ perm, int64_t N, const int64_t* __restrict__ cl_ptr, int64_t K, int32_t* status) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < N) {
    const int64_t r = perm[t];
    if (r < 0 || r >= N) atomicOr(status, FHVAE_KM_BAD_PERM);
  }
  if (t < K) {
    int64_t a, b;
    bool ok = km_cluster(cl_ptr, t, N, a, b);
    if (t == 0) ok = ok && a == 0;
    if (t == K - 1) ok = ok && b == N;
    if (!ok) atomicOr(status, FHVAE_KM_BAD_PTR);
  }
}

// pp[k] = the pieces of the clusters before k, pp[K] = all pieces: one workgroup; thread t sums a run of consecutive clusters,
// thread 0 turns the run totals into their prefix, every thread writes its run
__global__ void __launch_bounds__(kKmScan) km_piece_prefix_kernel(const int64_t* __restrict__ cl_ptr, int64_t K, int64_t N,
                                                                  int64_t* __restrict__ pp, const int32_t* status) {
  __shared__ int64_t run[kKmScan];
  if (*status & kKmBad) return;  // (set by the check kernel; the same in every thread)
  const int t = threadIdx.x;
  const int64_t per = (K + kKmScan - 1) / kKmScan, k0 = (int64_t)t * per, k1 = k0 + per < K ? k0 + per : K;
  int64_t s = 0;
  for (int64_t k = k0; k < k1; ++k) {
    int64_t a, b;
    if (km_cluster(cl_ptr, k, N, a, b)) s += km_pieces_of(b - a);
  }
  run[t] = s;
  __syncthreads();
  if (t == 0) {
    int64_t acc = 0;
    for (int j = 0; j < kKmScan; ++j) {
      const int64_t v = run[j];
      run[j] = acc;
      acc += v;
    }
  }
  __syncthreads();
  s = run[t];
  for (int64_t k = k0; k < k1; ++k) {
    pp[k] = s;
    int64_t a, b;
    if (km_cluster(cl_ptr, k, N, a, b)) s += km_pieces_of(b - a);
  }
  if (k0 < K && k1 == K) pp[K] = s;  // (K >= 1: exactly one thread's run holds the last cluster)
}

// the last k in [0, K) with pp[k] <= x; reads pp[0 .. K - 1] only
__device__ __forceinline__ int64_t km_find(const int64_t* __restrict__ pp, int64_t K, int64_t x) {
  int64_t lo = 0, hi = K - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (pp[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// 256 / D pieces per workgroup, one thread per (piece, column): 256 float64 additions in member order.  The thread of column 0
// also sums the piece's dist
__global__ void __launch_bounds__(256) km_piece_kernel(const float* __restrict__ x, int64_t ldx, int64_t N, int D,
                                                       const int64_t* __restrict__ perm, const int64_t* __restrict__ cl_ptr, int64_t K,
                                                       const float* __restrict__ dist, const int64_t* __restrict__ pp,
                                                       int64_t max_pieces, double* __restrict__ psum, double* __restrict__ pin,
                                                       const int32_t* status) {
  if (*status & kKmBad) return;
  const int per_wg = 256 / D, pl = threadIdx.x / D, d = threadIdx.x - pl * D;
  if (pl >= per_wg) return;
  const int64_t piece = (int64_t)blockIdx.x * per_wg + pl;
  if (piece >= max_pieces || piece >= pp[K]) return;
  const int64_t k = km_find(pp, K, piece);
  int64_t a, b;
  if (!km_cluster(cl_ptr, k, N, a, b)) return;
  const int64_t j = piece - pp[k];
  if (j < 0 || j >= km_pieces_of(b - a)) return;
  const int64_t m0 = a + j * kKmPiece, m1 = m0 + kKmPiece < b ? m0 + kKmPiece : b;
  double s = 0.0, si = 0.0;
  const bool inertia = d == 0 && dist != nullptr;
#pragma unroll 8
  for (int64_t m = m0; m < m1; ++m) {
    const int64_t r = perm[m];
    if (r < 0 || r >= N) continue;  // (the check kernel has refused it)
    s += (double)x[r * ldx + d];
    if (inertia) si += (double)dist[r];
  }
  psum[piece * D + d] = s;
  if (d == 0) pin[piece] = si;
}

// one thread per (k, d): the piece sums in piece order, the division, one rounding.  The thread of column 0 writes the count and
// the inertia
__global__ void km_combine_kernel(const int64_t* __restrict__ cl_ptr, int64_t K, int64_t N, int D, const int64_t* __restrict__ pp,
                                  int64_t max_pieces, const double* __restrict__ psum, const double* __restrict__ pin,
                                  float* __restrict__ cent, int64_t ldc, int64_t* __restrict__ count, double* __restrict__ cl_inertia,
                                  const int32_t* status) {
  if (*status & kKmBad) return;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= K * D) return;
  const int64_t k = e / D;
  const int d = (int)(e - k * D);
  int64_t a, b;
  if (!km_cluster(cl_ptr, k, N, a, b)) return;
  const int64_t c = b - a, np = km_pieces_of(c), p0 = pp[k];
  if (p0 < 0 || p0 > max_pieces - np) return;
  double s = 0.0, si = 0.0;
  for (int64_t j = 0; j < np; ++j) {
    s += psum[(p0 + j) * D + d];
    if (d == 0) si += pin[p0 + j];
  }
  if (c > 0) cent[k * ldc + d] = (float)(s / (double)c);
  if (d == 0) {
    count[k] = c;
    if (cl_inertia != nullptr) cl_inertia[k] = si;
  }
}

int km_check_args(const float* x, int64_t ldx, int64_t N, int64_t D, const float* cent, int64_t ldc, int64_t K, const void* ws,
                  int64_t ws_bytes) {
  FH_CHECK_PTR(x);
  FH_CHECK_PTR(cent);
  FH_CHECK_PTR(ws);
  FH_CHECK_POS(N);
  FH_CHECK_POS(K);
  int rc = fh_allpairs_check(x, ldx, D);
  if (rc != FHVAE_OK) return rc;
  rc = fh_allpairs_check(cent, ldc, D);
  if (rc != FHVAE_OK) return rc;
  if (((uintptr_t)ws & 15) != 0) return FHVAE_ERR_ALIGN;
  if (N > FHVAE_KM_MAX_ROWS || K > FHVAE_KM_MAX_CENT) return FHVAE_ERR_LIMIT;
  if (ws_bytes < km_ws(N, K, D).total) return FHVAE_ERR_SHAPE;
  return FHVAE_OK;
}

}  // namespace

}  // namespace fh

using namespace fh;

extern "C" int64_t fhvae_km_ws_bytes(int64_t N, int64_t K, int64_t D) {
  if (N < 1 || K < 1 || N > FHVAE_KM_MAX_ROWS || K > FHVAE_KM_MAX_CENT) return 0;
  if (D < 16 || D > 128 || D % 16 != 0) return 0;
  return km_ws(N, K, D).total;
}

extern "C" int fhvae_km_assign(const float* x, int64_t ldx, int64_t N, int64_t D, const float* cent, int64_t ldc, int64_t K, void* ws,
                               int64_t ws_bytes, int32_t* assign, float* dist, void* stream) {
  FH_CHECK_PTR(assign);
  int rc = km_check_args(x, ldx, N, D, cent, ldc, K, ws, ws_bytes);
  if (rc != FHVAE_OK) return rc;
  if (((uintptr_t)assign & 3) != 0 || ((uintptr_t)dist & 3) != 0) return FHVAE_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const KmWs w = km_ws(N, K, D);
  float* cn = (float*)((char*)ws + w.cn);
  float* xn = (float*)((char*)ws + w.xn);
  hipLaunchKernelGGL(km_sqnorm_kernel, dim3((unsigned)fh_cdiv(K, 256)), dim3(256), 0, st, cent, ldc, K, (int)D, cn);
  if (dist != nullptr) hipLaunchKernelGGL(km_sqnorm_kernel, dim3((unsigned)fh_cdiv(N, 256)), dim3(256), 0, st, x, ldx, N, (int)D, xn);
  rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  KmAssignArgs a = {};
  a.x = x;
  a.cent = cent;
  a.cn = cn;
  a.xn = xn;
  a.assign = assign;
  a.dist = dist;
  a.ldx = ldx;
  a.ldc = ldc;
  a.N = (int)N;
  a.K = (int)K;
  return fh_allpairs_dispatch(D, [&](auto d) { return km_assign_launch<decltype(d)::value>(a, st); });
}

extern "C" int fhvae_km_update(const float* x, int64_t ldx, int64_t N, int64_t D, const int64_t* perm, const int64_t* cl_ptr, int64_t K,
                               const float* dist, void* ws, int64_t ws_bytes, float* cent, int64_t ldc, int64_t* count,
                               double* cl_inertia, int32_t* status, void* stream) {
  FH_CHECK_PTR(perm);
  FH_CHECK_PTR(cl_ptr);
  FH_CHECK_PTR(count);
  FH_CHECK_PTR(status);
  int rc = km_check_args(x, ldx, N, D, cent, ldc, K, ws, ws_bytes);
  if (rc != FHVAE_OK) return rc;
  if (((uintptr_t)perm & 7) != 0 || ((uintptr_t)cl_ptr & 7) != 0 || ((uintptr_t)count & 7) != 0 || ((uintptr_t)cl_inertia & 7) != 0 ||
      ((uintptr_t)dist & 3) != 0 || ((uintptr_t)status & 3) != 0)
    return FHVAE_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const KmWs w = km_ws(N, K, D);
  int64_t* pp = (int64_t*)((char*)ws + w.pp);
  double* psum = (double*)((char*)ws + w.psum);
  double* pin = (double*)((char*)ws + w.pin);
  const int per_wg = 256 / (int)D;
  hipLaunchKernelGGL(km_check_kernel, dim3((unsigned)fh_cdiv(N > K ? N : K, 256)), dim3(256), 0, st, perm, N, cl_ptr, K, status);
  hipLaunchKernelGGL(km_piece_prefix_kernel, dim3(1), dim3(kKmScan), 0, st, cl_ptr, K, N, pp, status);
  hipLaunchKernelGGL(km_piece_kernel, dim3((unsigned)fh_cdiv(w.max_pieces, per_wg)), dim3(256), 0, st, x, ldx, N, (int)D, perm, cl_ptr, K,
                     dist, pp, w.max_pieces, psum, pin, status);
  hipLaunchKernelGGL(km_combine_kernel, dim3((unsigned)fh_cdiv(K * D, 256)), dim3(256), 0, st, cl_ptr, K, N, (int)D, pp, w.max_pieces, psum,
                     pin, cent, ldc, count, cl_inertia, status);
  return fh_launch_status();
}
