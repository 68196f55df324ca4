// gmm.hip -- a diagonal-covariance Gaussian mixture on (N, Dp) f32 rows (include/fhvae_gmm.h):
//   fhvae_gmm_loglik : every row's log-likelihood and its arg-max component;
//   fhvae_gmm_post   : every row's posteriors, from the log-likelihood of the call before;
//   fhvae_gmm_stats  : nk, sx, sxx of an EM step from the rows and their posteriors.
//
// The first two are allpairs_f32.h's pass, as km_assign_kernel uses it: a workgroup of 256 threads keeps 256 rows stationary and
// streams ALL K rows of the table through LDS in tiles of 64.  The stationary fragments are [x, x^2] of width W = 2 Dp: the
// half of a fragment that lies in [Dp, 2 Dp) is loaded from the same x and squared in registers, so no (N, 2 Dp) copy of the
// rows exists.  `side` puts the tile's cst beside it (-inf past K: a padded row has dot 0 and l = -inf, it never wins and adds
// nothing), `pair` turns a lane's four dots of a block into l and either keeps the online (m, s, bk) of the header (loglik) or
// writes expf(l - loglik) (post).  Both kernels are one template, so l has the same bits in both.
//
// The statistics are post^T . [x, x^2, 1] over the rows.  One workgroup takes (a slice of FHVAE_GMM_SLICE rows, 64 components), one
// wave 16 of the components; v_mfma_f32_16x16x4_f32 sums four rows per instruction.  Lane (g, i) supplies A = post[row + g][k0 + i]
// and B = x[row + g][c0 + i]: with row-major post and x both are 64 contiguous bytes per lane group, read straight from
// global memory, no LDS and no transposition.  The f32 partial of a (slice, component, column) goes to the workspace;
// gmm_combine_kernel adds a component's partials in slice order in float64.  No atomics anywhere.
//
// Arithmetic: exactly the header's.  No contraction (the pragma below and -ffp-contract=off).
#pragma clang fp contract(off)

#include <math.h>

#include "allpairs_f32.h"

#include "../../include/fhvae_gmm.h"

namespace fh {

namespace {

constexpr int kGmmYT = ap::kYT;
constexpr int kGmmSlice = FHVAE_GMM_SLICE;
constexpr int kGmmKT = 64;  // components per workgroup of the statistics: 16 per wave
constexpr int kGmmBatch = 32;  // partials whose loads the combine issues before it adds them

static_assert(kGmmYT == 64, "side() fills one cst per streamed row of a tile with the first 64 threads");
static_assert(kGmmSlice % 16 == 0, "the statistics step through a slice sixteen rows at a time");

struct GmmPassArgs {
  const float* x;
  const float* tab;
  const float* cst;     // (K)
  const float* ll_in;   // (N): post only
  float* loglik;        // (N): loglik only
  int32_t* label;       // (N) or nullptr: loglik only
  float* post;          // (N, K): post only
  int64_t ldx, ldt, ldp;
  int N, K;
};

// the stationary fragments [x, x^2] of a wave's 64 rows from x0 on (the layout of ap::load_stationary over W = 2 Dp columns): a
// 16-byte chunk lies wholly in one half (Dp is a multiple of 8); rows past nrows are zero
template <int W>
__device__ __forceinline__ void gmm_load_stationary(const float* __restrict__ x, int64_t ld, int nrows, int x0, uint4 (&xf)[4][W / 16]) {
  constexpr int Dp = W / 2;
  const int lane = threadIdx.x & 63, g = lane >> 4, i = lane & 15;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int r = x0 + t * 16 + i;
#pragma unroll
    for (int jj = 0; jj < W / 16; ++jj) {
      const int c = 16 * jj + 4 * g;
      const bool sq = c >= Dp;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < nrows) v = *(const float4*)(x + (int64_t)r * ld + (sq ? c - Dp : c));
      if (sq) v = make_float4(v.x * v.x, v.y * v.y, v.z * v.z, v.w * v.w);
      xf[t][jj] = make_uint4(__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w));
    }
  }
}

// (W > 96: 128 and more registers of stationary fragments; two workgroups per CU would spill, as in kmeans.hip)
template <int W, bool POST>
__global__ __launch_bounds__(256, W > 96 ? 1 : 2) void gmm_pass_kernel(GmmPassArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ytile = smem;                             // [64][W] f32, swizzled
  float* cstl = (float*)(smem + kGmmYT * W * 4);  // [64]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i = lane & 15;
  const int x0 = (int)blockIdx.x * 256 + wave * 64;  // (N <= 2^30: no overflow)
  const int K = a.K;

  uint4 xf[4][W / 16];
  gmm_load_stationary<W>(a.x, a.ldx, a.N, x0, xf);
  float m[4], s[4], ll[4];
  int bk[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    m[t] = -INFINITY, s[t] = 0.f, bk[t] = 0, ll[t] = 0.f;
    if (POST) {
      const int row = x0 + t * 16 + i;
      if (row < a.N) ll[t] = a.ll_in[row];
    }
  }

  ap::stream<W>(
      a.tab, a.ldt, 0, K, ytile, xf,
      [&](int y0) {
        if (tid < kGmmYT) cstl[tid] = y0 + tid < K ? a.cst[y0 + tid] : -INFINITY;
      },
      ap::EveryBlock(),
      [&](int y0, int yb, const f32x4(&acc)[4]) {
        const float4 cv = *(const float4*)(cstl + yb * 16 + 4 * g);
        const float cr[4] = {cv.x, cv.y, cv.z, cv.w};
        const int kb = y0 + yb * 16 + 4 * g;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          float l[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) l[r] = cr[r] + acc[t][r];
          if (POST) {
            const int row = x0 + t * 16 + i;
            if (row < a.N) {
              float* dst = a.post + (int64_t)row * a.ldp + kb;
              float p[4];
#pragma unroll
              for (int r = 0; r < 4; ++r) p[r] = expf(l[r] - ll[t]);
              if (kb + 3 < K) {
                *(float4*)dst = make_float4(p[0], p[1], p[2], p[3]);
              } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                  if (kb + r < K) dst[r] = p[r];
              }
            }
          } else {
            float b = m[t];
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (l[r] > b) b = l[r], bk[t] = kb + r;
            if (b > m[t]) s[t] = s[t] * expf(m[t] - b), m[t] = b;
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (l[r] != -INFINITY) s[t] = s[t] + expf(l[r] - m[t]);
          }
        }
      });

  if (POST) return;
  // ---- the four lanes of a row, in lane order: every lane of the row computes the same
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    float ma[4], sa[4];
    int ka[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      ma[q] = __shfl(m[t], i + 16 * q, 64);
      sa[q] = __shfl(s[t], i + 16 * q, 64);
      ka[q] = __shfl(bk[t], i + 16 * q, 64);
    }
    float M = ma[0];
    int kk = ka[0];
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      if (ma[q] > M || (ma[q] == M && ka[q] < kk)) kk = ka[q];
      if (ma[q] > M) M = ma[q];
    }
    float S = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) S = S + (sa[q] == 0.f ? 0.f : sa[q] * expf(ma[q] - M));
    const int row = x0 + t * 16 + i;
    if (g == 0 && row < a.N) {
      a.loglik[row] = M + logf(S);
      if (a.label != nullptr) a.label[row] = kk;
    }
  }
}

template <int W, bool POST>
int gmm_pass_launch(const GmmPassArgs& a, hipStream_t st) {
  const int smem = kGmmYT * W * 4 + kGmmYT * 4;
  hipLaunchKernelGGL((gmm_pass_kernel<W, POST>), dim3((unsigned)fh_cdiv(a.N, 256)), dim3(256), (size_t)smem, st, a);
  return fh_launch_status();
}

// ---- statistics
// partial (slices, K, P) f32, P = 2 Dp + 1: columns [0, Dp) sx, [Dp, 2 Dp) sxx, 2 Dp nk
inline int64_t gmm_slices(int64_t N) { return fh_cdiv(N, kGmmSlice); }
inline int64_t gmm_ws(int64_t N, int64_t K, int64_t Dp) { return fh_cdiv(gmm_slices(N) * K * (2 * Dp + 1) * 4, 256) * 256; }

// NB = the blocks of 16 columns that cover Dp.  grid (slices, tiles of 64 components); wave w takes components k0 .. k0 + 15
template <int NB>
__global__ __launch_bounds__(256) void gmm_stats_kernel(const float* __restrict__ x, int64_t ldx, int N, int Dp,
                                                        const float* __restrict__ post, int64_t ldp, int K, float* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, i = lane & 15;
  const int k0 = (int)blockIdx.y * kGmmKT + wave * 16;
  if (k0 >= K) return;  // (uniform over the wave; the kernel has no barrier)
  const int64_t slice = blockIdx.x;
  const int n0 = (int)(slice * kGmmSlice);  // (N <= 2^30: no overflow)
  const int n1 = n0 + kGmmSlice < N ? n0 + kGmmSlice : N;
  const bool kin = k0 + i < K;

  f32x4 ax[NB], aq[NB], a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int b = 0; b < NB; ++b) ax[b] = f32x4{0.f, 0.f, 0.f, 0.f}, aq[b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // 16 rows per trip, so that four steps' loads are in flight; a row from n1 on enters as 0 * 0, which changes no sum
  for (int n = n0; n < n1; n += 16) {
    float p[4], xv[4][NB];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = n + 4 * u + g;
      const bool in = row < n1;
      p[u] = (in && kin) ? post[(int64_t)row * ldp + k0 + i] : 0.f;
#pragma unroll
      for (int b = 0; b < NB; ++b) xv[u][b] = (in && 16 * b + i < Dp) ? x[(int64_t)row * ldx + 16 * b + i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        ax[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[u], xv[u][b], ax[b], 0, 0, 0);
        aq[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[u], xv[u][b] * xv[u][b], aq[b], 0, 0, 0);
      }
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(p[u], 1.f, a1, 0, 0, 0);
    }
  }

  // acc[r] is (component k0 + 4 g + r, column 16 b + i)
  const int P = 2 * Dp + 1;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = k0 + 4 * g + r;
    if (k >= K) continue;
    float* dst = part + (slice * K + k) * P;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int c = 16 * b + i;
      if (c < Dp) dst[c] = ax[b][r], dst[Dp + c] = aq[b][r];
    }
    if (i == 0) dst[2 * Dp] = a1[r];
  }
}

// one thread per (k, column): the partials in slice order in float64, onto what the output holds if `accumulate`
__global__ void gmm_combine_kernel(const float* __restrict__ part, int64_t slices, int64_t K, int Dp, double* __restrict__ nk,
                                   double* __restrict__ sx, double* __restrict__ sxx, int accumulate) {
  const int P = 2 * Dp + 1;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= K * P) return;
  const int64_t k = e / P;
  const int c = (int)(e - k * P);
  double* out = c < Dp ? sx + k * Dp + c : (c < 2 * Dp ? sxx + k * Dp + (c - Dp) : nk + k);
  double v = accumulate ? *out : 0.0;
  // the additions are one chain in slice order; the loads of kGmmBatch slices fly together ahead of it
  const float* src = part + e;
  const int64_t stride = K * P;
  int64_t sl = 0;
  for (; sl + kGmmBatch <= slices; sl += kGmmBatch) {
    float p[kGmmBatch];
#pragma unroll
    for (int j = 0; j < kGmmBatch; ++j) p[j] = src[(sl + j) * stride];
#pragma unroll
    for (int j = 0; j < kGmmBatch; ++j) v += (double)p[j];
  }
  for (; sl < slices; ++sl) v += (double)src[sl * stride];
  *out = v;
}

int gmm_check_rows(const float* x, int64_t ldx, int64_t N, int64_t Dp, int64_t K) {
  FH_CHECK_PTR(x);
  FH_CHECK_POS(N);
  FH_CHECK_POS(K);
  if (Dp < 8 || Dp > FHVAE_GMM_MAX_DP || Dp % 8 != 0) return FHVAE_ERR_SHAPE;
  if (ldx < Dp) return FHVAE_ERR_SHAPE;
  return FHVAE_OK;
}

// a (rows, width) f32 matrix: after the shapes of every argument, before the limits
inline bool gmm_misaligned(const void* p, int64_t ld) { return ld % 4 != 0 || ((uintptr_t)p & 15) != 0; }

int gmm_check_pass(const float* x, int64_t ldx, int64_t N, int64_t Dp, const float* tab, int64_t ldt, const float* cst, int64_t K) {
  FH_CHECK_PTR(tab);
  FH_CHECK_PTR(cst);
  int rc = gmm_check_rows(x, ldx, N, Dp, K);
  if (rc != FHVAE_OK) return rc;
  if (ldt < 2 * Dp) return FHVAE_ERR_SHAPE;
  if (gmm_misaligned(x, ldx) || gmm_misaligned(tab, ldt) || ((uintptr_t)cst & 3) != 0) return FHVAE_ERR_ALIGN;
  return FHVAE_OK;
}

inline int gmm_check_limits(int64_t N, int64_t K) { return (N > FHVAE_GMM_MAX_ROWS || K > FHVAE_GMM_MAX_COMP) ? FHVAE_ERR_LIMIT : FHVAE_OK; }

}  // namespace

}  // namespace fh

using namespace fh;

extern "C" int64_t fhvae_gmm_ws_bytes(int64_t N, int64_t K, int64_t Dp) {
  if (N < 1 || K < 1 || N > FHVAE_GMM_MAX_ROWS || K > FHVAE_GMM_MAX_COMP) return 0;
  if (Dp < 8 || Dp > FHVAE_GMM_MAX_DP || Dp % 8 != 0) return 0;
  return gmm_ws(N, K, Dp);
}

extern "C" int fhvae_gmm_loglik(const float* x, int64_t ldx, int64_t N, int64_t Dp, const float* tab, int64_t ldt, const float* cst,
                                int64_t K, float* loglik, int32_t* label, void* stream) {
  FH_CHECK_PTR(loglik);
  int rc = gmm_check_pass(x, ldx, N, Dp, tab, ldt, cst, K);
  if (rc != FHVAE_OK) return rc;
  if (((uintptr_t)loglik & 3) != 0 || ((uintptr_t)label & 3) != 0) return FHVAE_ERR_ALIGN;
  rc = gmm_check_limits(N, K);
  if (rc != FHVAE_OK) return rc;
  GmmPassArgs a = {};
  a.x = x, a.tab = tab, a.cst = cst, a.loglik = loglik, a.label = label;
  a.ldx = ldx, a.ldt = ldt, a.N = (int)N, a.K = (int)K;
  hipStream_t st = (hipStream_t)stream;
  return fh_allpairs_dispatch(2 * Dp, [&](auto w) { return gmm_pass_launch<decltype(w)::value, false>(a, st); });
}

extern "C" int fhvae_gmm_post(const float* x, int64_t ldx, int64_t N, int64_t Dp, const float* tab, int64_t ldt, const float* cst,
                              int64_t K, const float* loglik, float* post, int64_t ldp, void* stream) {
  FH_CHECK_PTR(loglik);
  FH_CHECK_PTR(post);
  int rc = gmm_check_pass(x, ldx, N, Dp, tab, ldt, cst, K);
  if (rc != FHVAE_OK) return rc;
  if (ldp < K) return FHVAE_ERR_SHAPE;
  if (((uintptr_t)loglik & 3) != 0 || gmm_misaligned(post, ldp)) return FHVAE_ERR_ALIGN;
  rc = gmm_check_limits(N, K);
  if (rc != FHVAE_OK) return rc;
  GmmPassArgs a = {};
  a.x = x, a.tab = tab, a.cst = cst, a.ll_in = loglik, a.post = post;
  a.ldx = ldx, a.ldt = ldt, a.ldp = ldp, a.N = (int)N, a.K = (int)K;
  hipStream_t st = (hipStream_t)stream;
  return fh_allpairs_dispatch(2 * Dp, [&](auto w) { return gmm_pass_launch<decltype(w)::value, true>(a, st); });
}

extern "C" int fhvae_gmm_stats(const float* x, int64_t ldx, int64_t N, int64_t Dp, const float* post, int64_t ldp, int64_t K, void* ws,
                               int64_t ws_bytes, double* nk, double* sx, double* sxx, int accumulate, void* stream) {
  FH_CHECK_PTR(post);
  FH_CHECK_PTR(ws);
  FH_CHECK_PTR(nk);
  FH_CHECK_PTR(sx);
  FH_CHECK_PTR(sxx);
  int rc = gmm_check_rows(x, ldx, N, Dp, K);
  if (rc != FHVAE_OK) return rc;
  if (ldp < K) return FHVAE_ERR_SHAPE;
  if (gmm_misaligned(x, ldx) || gmm_misaligned(post, ldp) || ((uintptr_t)ws & 15) != 0 || ((uintptr_t)nk & 7) != 0 ||
      ((uintptr_t)sx & 7) != 0 || ((uintptr_t)sxx & 7) != 0)
    return FHVAE_ERR_ALIGN;
  rc = gmm_check_limits(N, K);
  if (rc != FHVAE_OK) return rc;
  if (ws_bytes < gmm_ws(N, K, Dp)) return FHVAE_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  const int64_t slices = gmm_slices(N);
  const dim3 grid((unsigned)slices, (unsigned)fh_cdiv(K, kGmmKT));
  switch (fh_cdiv(Dp, 16)) {
    case 1: hipLaunchKernelGGL(gmm_stats_kernel<1>, grid, dim3(256), 0, st, x, ldx, (int)N, (int)Dp, post, ldp, (int)K, part); break;
    case 2: hipLaunchKernelGGL(gmm_stats_kernel<2>, grid, dim3(256), 0, st, x, ldx, (int)N, (int)Dp, post, ldp, (int)K, part); break;
    case 3: hipLaunchKernelGGL(gmm_stats_kernel<3>, grid, dim3(256), 0, st, x, ldx, (int)N, (int)Dp, post, ldp, (int)K, part); break;
    default: hipLaunchKernelGGL(gmm_stats_kernel<4>, grid, dim3(256), 0, st, x, ldx, (int)N, (int)Dp, post, ldp, (int)K, part); break;
  }
  rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  hipLaunchKernelGGL(gmm_combine_kernel, dim3((unsigned)fh_cdiv(K * (2 * Dp + 1), 256)), dim3(256), 0, st, part, slices, K, (int)Dp, nk,
                     sx, sxx, accumulate);
  return fh_launch_status();
}
