// ivector.hip -- i-vector extraction (include/fhvae_ivector.h):
//   fhvae_iv_stats : n_c(u), f_c(u) of every utterance of a batch from the rows and their posteriors, in one launch;
//   fhvae_iv_solve : per utterance the float64 root-free Cholesky factor of its packed posterior precision, w = L^-1 b, log det L and
//                    E = L^-1 + w w^T.
//
// The statistics are gmm.hip's post^T . [x, 1] product, cut per utterance.  The utterances' pointers live on the device, so the
// host cannot know the slices: iv_plan_kernel (one workgroup) writes the exclusive prefix `off` of the utterances' slice counts
// into the workspace, and the grid of iv_stats_kernel is (N / SLICE + U work items, tiles of 64 components): item w finds its
// (utterance, slice) by a binary search of `off`, and an item past off[U] has nothing to do.  One wave takes 16 components;
// lane (g, i) supplies A = post[row + g][k0 + i] and B = x[row + g][c0 + i] to v_mfma_f32_16x16x4_f32, both read straight from
// global memory (gmm.hip's layout; the slice product is written beside gmm.hip's, whose code is untouched).  The f32 partial of an
// (item, component, column) goes to the workspace; iv_combine_kernel adds an utterance's partials in slice order in float64 and
// rounds once.  No atomics on floating-point values anywhere.
//
// The solve keeps the packed triangle in LDS (66 048 bytes at R = 128) and gives every chain of the header to one thread: TPU
// threads per utterance (32, 64 or 128: the smallest that is at least R, so that a thread owns a row), 256 / TPU utterances per
// workgroup at R <= 64 and one workgroup of 128 threads per utterance above (two of them fit a CU's LDS).  All loop bounds depend
// on R alone, so every barrier is met by the whole workgroup; an utterance whose pivot fails goes on computing NaN.
//
// Arithmetic: exactly the header's.  No contraction (the pragma below and -ffp-contract=off); the fused operations are explicit fma.
#pragma clang fp contract(off)

#include <math.h>

#include "common.h"

#include "../../include/fhvae_ivector.h"

namespace fh {

namespace {

constexpr int kIvSlice = FHVAE_IV_SLICE;
constexpr int kIvKT = 64;      // components per workgroup of the statistics: 16 per wave
constexpr int kIvBatch = 32;   // partials whose loads the combine issues before it adds them
constexpr int kIvPlanT = 1024; // threads of the plan's one workgroup

static_assert(kIvSlice % 16 == 0, "the statistics step through a slice sixteen rows at a time");

inline int64_t iv_items(int64_t N, int64_t U) { return fh_cdiv(N, kIvSlice) + U; }
inline int64_t iv_off_bytes(int64_t U) { return fh_cdiv((U + 1) * 8, 256) * 256; }
inline int64_t iv_ws(int64_t N, int64_t U, int64_t C, int64_t Dp) {
  return iv_off_bytes(U) + fh_cdiv(iv_items(N, U) * C * (Dp + 1) * 4, 256) * 256;
}

// the slices of utterance u, or -1 when it is not good
__device__ __forceinline__ int64_t iv_count(const int64_t* __restrict__ ptr, int64_t u, int64_t N) {
  const int64_t a = ptr[u], b = ptr[u + 1];
  if (a < 0 || b < a || b > N) return -1;
  return (b - a + kIvSlice - 1) / kIvSlice;
}

// off (U + 1): the exclusive prefix of the good utterances' slice counts.  One workgroup; thread t owns a run of consecutive
// utterances.  An utterance whose slices end past `cap` is left out by the kernels below (off[u + 1] > cap) and reported here.
__global__ __launch_bounds__(kIvPlanT) void iv_plan_kernel(const int64_t* __restrict__ ptr, int64_t U, int64_t N, int64_t cap,
                                                           int64_t* __restrict__ off, int32_t* __restrict__ status) {
  __shared__ int64_t sums[kIvPlanT];
  const int t = threadIdx.x;
  const int64_t run = (U + kIvPlanT - 1) / kIvPlanT;
  const int64_t lo = (int64_t)t * run < U ? (int64_t)t * run : U, hi = lo + run < U ? lo + run : U;
  int64_t s = 0;
  bool bad = false;
  for (int64_t u = lo; u < hi; ++u) {
    const int64_t c = iv_count(ptr, u, N);
    if (c < 0) bad = true; else s += c;
  }
  sums[t] = s;
  __syncthreads();
  if (t == 0) {
    int64_t acc = 0;
    for (int j = 0; j < kIvPlanT; ++j) {
      const int64_t v = sums[j];
      sums[j] = acc;
      acc += v;
    }
  }
  __syncthreads();
  int64_t at = sums[t];
  for (int64_t u = lo; u < hi; ++u) {
    off[u] = at;
    const int64_t c = iv_count(ptr, u, N);
    if (c > 0) at += c;
    if (c > 0 && at > cap) bad = true;
  }
  if (hi == U && lo < hi) off[U] = at;
  if (bad) atomicOr(status, (int32_t)FHVAE_IV_BAD_PTR);
}

// NB = the blocks of 16 columns that cover Dp.  grid (work items, tiles of 64 components); wave w takes components k0 .. k0 + 15.
// part (items, C, Dp + 1) f32: columns [0, Dp) f, column Dp n
template <int NB>
__global__ __launch_bounds__(256) void iv_stats_kernel(const float* __restrict__ x, int64_t ldx, int N, int Dp, const float* __restrict__ post,
                                                       int64_t ldp, int C, const int64_t* __restrict__ ptr, int64_t U,
                                                       const int64_t* __restrict__ off, int64_t cap, float* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, i = lane & 15;
  const int k0 = (int)blockIdx.y * kIvKT + wave * 16;
  if (k0 >= C) return;  // (uniform over the wave; the kernel has no barrier)
  const int64_t item = blockIdx.x;
  if (item >= cap || item >= off[U]) return;
  // the utterance: the last u with off[u] <= item (equal offsets: empty or bad utterances before it)
  int64_t lo = 0, hi = U;  // off[lo] <= item < off[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= item) lo = mid; else hi = mid;
  }
  const int64_t u = lo;
  if (off[u + 1] > cap) return;  // (its slices do not fit the workspace: the combine writes zeros)
  const int64_t a = ptr[u], b = ptr[u + 1];
  if (a < 0 || b < a || b > N) return;  // (re-checked: the plan counted no slice for it)
  const int64_t first = a + (item - off[u]) * kIvSlice;
  if (first >= b) return;
  const int n0 = (int)first;  // (N <= 2^30: no overflow)
  const int n1 = first + kIvSlice < b ? n0 + kIvSlice : (int)b;
  const bool kin = k0 + i < C;

  f32x4 ax[NB], a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int bb = 0; bb < NB; ++bb) ax[bb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // 16 rows per trip, so that four steps' loads are in flight; a row from n1 on enters as 0 * 0, which changes no sum
  for (int n = n0; n < n1; n += 16) {
    float p[4], xv[4][NB];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int row = n + 4 * s + g;
      const bool in = row < n1;
      p[s] = (in && kin) ? post[(int64_t)row * ldp + k0 + i] : 0.f;
#pragma unroll
      for (int bb = 0; bb < NB; ++bb) xv[s][bb] = (in && 16 * bb + i < Dp) ? x[(int64_t)row * ldx + 16 * bb + i] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int bb = 0; bb < NB; ++bb) ax[bb] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[s], xv[s][bb], ax[bb], 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(p[s], 1.f, a1, 0, 0, 0);
    }
  }

  // acc[r] is (component k0 + 4 g + r, column 16 bb + i)
  const int P = Dp + 1;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = k0 + 4 * g + r;
    if (k >= C) continue;
    float* dst = part + (item * C + k) * P;
#pragma unroll
    for (int bb = 0; bb < NB; ++bb) {
      const int c = 16 * bb + i;
      if (c < Dp) dst[c] = ax[bb][r];
    }
    if (i == 0) dst[Dp] = a1[r];
  }
}

// one thread per (u, component, column): the utterance's partials in slice order in float64, rounded once
__global__ void iv_combine_kernel(const float* __restrict__ part, const int64_t* __restrict__ off, int64_t cap, int64_t U, int64_t C,
                                  int Dp, float* __restrict__ nout, float* __restrict__ fout) {
  const int P = Dp + 1;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= U * C * P) return;
  const int64_t u = e / (C * P);
  const int64_t kc = e - u * (C * P);
  const int64_t k = kc / P;
  const int c = (int)(kc - k * P);
  int64_t s0 = off[u], s1 = off[u + 1];
  if (s0 < 0 || s1 < s0 || s1 > cap) s1 = s0 = 0;
  double v = 0.0;
  const float* src = part + kc;
  const int64_t stride = C * P;
  int64_t sl = s0;
  for (; sl + kIvBatch <= s1; sl += kIvBatch) {
    float p[kIvBatch];
#pragma unroll
    for (int j = 0; j < kIvBatch; ++j) p[j] = src[(sl + j) * stride];
#pragma unroll
    for (int j = 0; j < kIvBatch; ++j) v += (double)p[j];
  }
  for (; sl < s1; ++sl) v += (double)src[sl * stride];
  if (c < Dp) fout[(u * C + k) * Dp + c] = (float)v; else nout[u * C + k] = (float)v;
}

// ---- solve
__device__ __forceinline__ int iv_tri(int i) { return i * (i + 1) / 2; }

// TPU threads per utterance, UPB utterances per workgroup of TPU * UPB threads.  LDS per utterance: P + 2 R doubles (the triangle:
// G below the diagonal, d on it; y; the scaled row u of the column in hand) and one flag
template <int TPU, int UPB>
__global__ __launch_bounds__(TPU * UPB) void iv_solve_kernel(const double* __restrict__ Lp, const double* __restrict__ b, int64_t U, int R,
                                                             double* __restrict__ w, double* __restrict__ E, double* __restrict__ logdet,
                                                             int32_t* __restrict__ status) {
  extern __shared__ double iv_lds[];
  const int P = iv_tri(R);
  const int per = P + 2 * R;
  const int slot = threadIdx.x / TPU, t = threadIdx.x % TPU;
  const int64_t u = (int64_t)blockIdx.x * UPB + slot;
  const bool active = u < U;
  double* tri = iv_lds + (size_t)slot * per;
  double* yv = tri + P;
  double* uv = yv + R;
  int* flags = (int*)(iv_lds + (size_t)UPB * per);

  if (active) {
    for (int p = t; p < P; p += TPU) tri[p] = Lp[u * P + p];
    for (int j = t; j < R; j += TPU) yv[j] = b[u * R + j];
  }
  if (t == 0) flags[slot] = 0;
  __syncthreads();

  const bool row = active && t < R;  // thread t owns row t
  const int ti = iv_tri(t);
  // 1. L = G D G^T, column by column; uv holds u_k = G[j][k] * d_k of the column j in hand
  for (int j = 0; j < R; ++j) {
    const int tj = iv_tri(j);
    double acc = 0.0;
    if (row && t >= j) {
      acc = tri[ti + j];
      for (int k = 0; k < j; ++k) acc = fma(-tri[ti + k], uv[k], acc);
      if (t == j) {
        if (!(acc > 0.0) || !(acc < INFINITY)) flags[slot] = 1;
        tri[tj + j] = acc;
      }
    }
    __syncthreads();
    if (row) {
      const double d = tri[tj + j];
      if (t > j) {
        const double g = acc / d;
        tri[ti + j] = g;
        if (t == j + 1) uv[j] = g * d;
      } else if (t < j && j + 1 < R) {
        uv[t] = tri[iv_tri(j + 1) + t] * tri[ti + t];
      }
    }
    __syncthreads();
  }
  // 2. z = G^-1 b, y = D^-1 z, w = G^-T y
  for (int j = 0; j < R; ++j) {
    if (row && t > j) yv[t] = fma(-tri[ti + j], yv[j], yv[t]);
    __syncthreads();
  }
  if (row) yv[t] = yv[t] / tri[ti + t];
  __syncthreads();
  for (int k = R - 1; k > 0; --k) {
    if (row && t < k) yv[t] = fma(-tri[iv_tri(k) + t], yv[k], yv[t]);
    __syncthreads();
  }
  const bool failed = flags[slot] != 0;
  const double nan = __builtin_nan("");
  if (active) {
    for (int j = t; j < R; j += TPU) w[u * R + j] = failed ? nan : yv[j];
    if (t == 0) {
      // 3. log det
      if (logdet != nullptr) {
        double s = 0.0;
        for (int j = 0; j < R; ++j) s = s + log(tri[iv_tri(j) + j]);
        logdet[u] = failed ? nan : s;
      }
      if (failed) atomicOr(status, (int32_t)FHVAE_IV_NOT_PD);
    }
  }
  if (E == nullptr) return;  // (uniform over the workgroup)
  __syncthreads();           // (the diagonal is read above and rewritten below)
  // 4. H = G^-1 in place, row by row: thread t owns column t of the row; the diagonal becomes 1 / d
  for (int i = 0; i < R; ++i) {
    const int tr = iv_tri(i);
    double val = 0.0;
    if (active && t <= i) {
      if (t == i) {
        val = 1.0 / tri[tr + i];
      } else {
        double acc = tri[tr + t];
        for (int k = t + 1; k < i; ++k) acc = fma(tri[tr + k], tri[iv_tri(k) + t], acc);
        val = -acc;
      }
    }
    __syncthreads();
    if (active && t <= i) tri[tr + t] = val;
    __syncthreads();
  }
  if (!active) return;
  // E = H^T D^-1 H + w w^T, one thread per packed entry
  for (int p = t; p < P; p += TPU) {
    int i = (int)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while (iv_tri(i + 1) <= p) ++i;
    while (iv_tri(i) > p) --i;
    const int j = p - iv_tri(i);
    // k = i: H[i][i] = 1
    double s = j == i ? tri[iv_tri(i) + i] : tri[iv_tri(i) + i] * tri[iv_tri(i) + j];
    for (int k = i + 1; k < R; ++k) {
      const int tk = iv_tri(k);
      s = fma(tri[tk + i] * tri[tk + k], tri[tk + j], s);
    }
    E[u * P + p] = failed ? nan : fma(yv[i], yv[j], s);
  }
}

template <int TPU, int UPB>
int iv_solve_launch(const double* Lp, const double* b, int64_t U, int R, double* w, double* E, double* logdet, int32_t* status,
                    hipStream_t st) {
  const int P = R * (R + 1) / 2;
  const int smem = UPB * (P + 2 * R) * 8 + UPB * 4;  // (the triangle, y, u)
  hipError_t e = hipFuncSetAttribute((const void*)iv_solve_kernel<TPU, UPB>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((iv_solve_kernel<TPU, UPB>), dim3((unsigned)fh_cdiv(U, UPB)), dim3(TPU * UPB), (size_t)smem, st, Lp, b, U, R, w, E,
                     logdet, status);
  return fh_launch_status();
}

inline bool iv_dp_ok(int64_t Dp) { return Dp >= 8 && Dp <= 64 && Dp % 8 == 0; }

}  // namespace

}  // namespace fh

using namespace fh;

extern "C" int64_t fhvae_iv_ws_bytes(int64_t N, int64_t U, int64_t C, int64_t Dp) {
  if (N < 1 || U < 1 || C < 1 || N > FHVAE_IV_MAX_ROWS || U > FHVAE_IV_MAX_UTT || C > FHVAE_IV_MAX_COMP) return 0;
  if (!iv_dp_ok(Dp)) return 0;
  return iv_ws(N, U, C, Dp);
}

extern "C" int fhvae_iv_stats(const float* x, int64_t ldx, int64_t N, int64_t Dp, const float* post, int64_t ldp, int64_t C,
                              const int64_t* utt_ptr, int64_t U, void* ws, int64_t ws_bytes, float* n, float* f, int32_t* status,
                              void* stream) {
  FH_CHECK_PTR(x);
  FH_CHECK_PTR(post);
  FH_CHECK_PTR(utt_ptr);
  FH_CHECK_PTR(ws);
  FH_CHECK_PTR(n);
  FH_CHECK_PTR(f);
  FH_CHECK_PTR(status);
  FH_CHECK_POS(N);
  FH_CHECK_POS(U);
  FH_CHECK_POS(C);
  if (!iv_dp_ok(Dp)) return FHVAE_ERR_SHAPE;
  if (ldx < Dp || ldp < C) return FHVAE_ERR_SHAPE;
  if (ldx % 4 != 0 || ldp % 4 != 0 || ((uintptr_t)x & 15) != 0 || ((uintptr_t)post & 15) != 0 || ((uintptr_t)ws & 15) != 0 ||
      ((uintptr_t)utt_ptr & 7) != 0 || ((uintptr_t)n & 3) != 0 || ((uintptr_t)f & 3) != 0 || ((uintptr_t)status & 3) != 0)
    return FHVAE_ERR_ALIGN;
  if (N > FHVAE_IV_MAX_ROWS || U > FHVAE_IV_MAX_UTT || C > FHVAE_IV_MAX_COMP) return FHVAE_ERR_LIMIT;
  if (U * C * (Dp + 1) > ((int64_t)1 << 39)) return FHVAE_ERR_LIMIT;  // (the combine's grid: one thread per output entry)
  if (ws_bytes < iv_ws(N, U, C, Dp)) return FHVAE_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  int64_t* off = (int64_t*)ws;
  float* part = (float*)((char*)ws + iv_off_bytes(U));
  const int64_t cap = iv_items(N, U);
  hipLaunchKernelGGL(iv_plan_kernel, dim3(1), dim3(kIvPlanT), 0, st, utt_ptr, U, N, cap, off, status);
  int rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  const dim3 grid((unsigned)cap, (unsigned)fh_cdiv(C, kIvKT));
  switch (fh_cdiv(Dp, 16)) {
    case 1: hipLaunchKernelGGL(iv_stats_kernel<1>, grid, dim3(256), 0, st, x, ldx, (int)N, (int)Dp, post, ldp, (int)C, utt_ptr, U, off, cap, part); break;
    case 2: hipLaunchKernelGGL(iv_stats_kernel<2>, grid, dim3(256), 0, st, x, ldx, (int)N, (int)Dp, post, ldp, (int)C, utt_ptr, U, off, cap, part); break;
    case 3: hipLaunchKernelGGL(iv_stats_kernel<3>, grid, dim3(256), 0, st, x, ldx, (int)N, (int)Dp, post, ldp, (int)C, utt_ptr, U, off, cap, part); break;
    default: hipLaunchKernelGGL(iv_stats_kernel<4>, grid, dim3(256), 0, st, x, ldx, (int)N, (int)Dp, post, ldp, (int)C, utt_ptr, U, off, cap, part); break;
  }
  rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  hipLaunchKernelGGL(iv_combine_kernel, dim3((unsigned)fh_cdiv(U * C * (Dp + 1), 256)), dim3(256), 0, st, part, off, cap, U, C, (int)Dp, n, f);
  return fh_launch_status();
}

extern "C" int fhvae_iv_solve(const double* Lp, const double* b, int64_t U, int64_t R, double* w, double* E, double* logdet,
                              int32_t* status, void* stream) {
  FH_CHECK_PTR(Lp);
  FH_CHECK_PTR(b);
  FH_CHECK_PTR(w);
  FH_CHECK_PTR(status);
  FH_CHECK_POS(U);
  FH_CHECK_POS(R);
  if (((uintptr_t)Lp & 7) != 0 || ((uintptr_t)b & 7) != 0 || ((uintptr_t)w & 7) != 0 || ((uintptr_t)E & 7) != 0 ||
      ((uintptr_t)logdet & 7) != 0 || ((uintptr_t)status & 3) != 0)
    return FHVAE_ERR_ALIGN;
  if (R > FHVAE_IV_MAX_RANK || U > FHVAE_IV_MAX_UTT) return FHVAE_ERR_LIMIT;
  hipStream_t st = (hipStream_t)stream;
  if (R <= 32) return iv_solve_launch<32, 8>(Lp, b, U, (int)R, w, E, logdet, status, st);
  if (R <= 64) return iv_solve_launch<64, 4>(Lp, b, U, (int)R, w, E, logdet, status, st);
  return iv_solve_launch<128, 1>(Lp, b, U, (int)R, w, E, logdet, status, st);
}
