// probe.hip -- a linear probe (multinomial logistic regression) on (N, W) f32 rows (include/fhvae_probe.h):
//   fhvae_probe_rows : every row's log-sum-exp, arg-max class and negative log-likelihood, and their float64 totals;
//   fhvae_probe_grad : the gradient of the summed negative log-likelihood, (C, W + 1) float64, with no (N, C) array.
//
// Pass 1 is allpairs_f32.h's pass as gmm_pass_kernel uses it: a workgroup of 256 threads keeps 256 rows stationary and streams ALL
// C rows of the table through LDS in tiles of 64; `side` puts the tile's cst beside it (-inf past C), `pair` turns a lane's four
// dots of a block into l, keeps the online (m, s, bc) of the header and picks l(n, y[n]) up as it passes.
//
// Pass 2 turns the pass round: a workgroup owns (a slice of FHVAE_PROBE_SLICE rows, 64 T classes), a wave 16 T of the classes as
// its STATIONARY fragments, and the slice's rows stream through LDS.  The dot tile acc[t][r] = dot(class c0 + 16 t + i, row
// b + 4 g + r) is, after r = expf(cst + dot - lse) - onehot on the VALU, exactly the B operand (k = g, n = i) of a second
// v_mfma_f32_16x16x4_f32 whose A operand is column d = 16 dj + i of the rows b + 4 g + r, read from the same LDS tile (1 for the
// bias column): MFMA r of a block sums the rows {b + 4 g + r}.  The residual never leaves registers.  The f32 partial of a
// (slice, class, column) goes to the workspace; probe_combine_kernel adds them in slice order in float64.  No atomics anywhere.
// Because dot(i, j) == dot(j, i) bit for bit (allpairs_f32.h), l has the same bits in both passes.
//
// Arithmetic: exactly the header's.  No contraction (the pragma below and -ffp-contract=off).
#pragma clang fp contract(off)

#include <math.h>

#include "allpairs_f32.h"

#include "../../include/fhvae_probe.h"

namespace fh {

namespace {

constexpr int kPrYT = ap::kYT;
constexpr int kPrSlice = FHVAE_PROBE_SLICE;
constexpr int kPrBatch = 32;  // partials whose loads the combine issues before it adds them

static_assert(kPrYT == 64, "side() fills one value per streamed row of a tile with the first 64 threads");
static_assert(kPrSlice % kPrYT == 0, "a slice is whole tiles");

struct ProbeArgs {
  const float* x;
  const float* tab;
  const float* cst;      // (C)
  const int32_t* y;      // (N)
  const float* lse_in;   // (N): pass 2
  float* lse;            // (N): pass 1
  int32_t* pred;         // (N): pass 1
  float* nll;            // (N): pass 1
  float* part;           // (slices, C, W + 1): pass 2
  int64_t ldx, ldt;
  int N, C;
};

// ---- pass 1
// (W > 96: 128 and more registers of stationary fragments; two workgroups per CU would spill, as in gmm.hip)
template <int W>
__global__ __launch_bounds__(256, W > 96 ? 1 : 2) void probe_rows_kernel(ProbeArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ytile = smem;                            // [64][W] f32, swizzled
  float* cstl = (float*)(smem + kPrYT * W * 4);  // [64]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i = lane & 15;
  const int x0 = (int)blockIdx.x * 256 + wave * 64;  // (N <= 2^30: no overflow)
  const int C = a.C;

  uint4 xf[4][W / 16];
  ap::load_stationary<W>(a.x, a.ldx, a.N, x0, xf);
  float m[4], s[4], ly[4];
  int bc[4], yv[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    m[t] = -INFINITY, s[t] = 0.f, bc[t] = 0, ly[t] = 0.f, yv[t] = -1;
    const int row = x0 + t * 16 + i;
    if (row < a.N) {
      const int v = a.y[row];
      if ((unsigned)v < (unsigned)C) yv[t] = v;
    }
  }

  ap::stream<W>(
      a.tab, a.ldt, 0, C, ytile, xf,
      [&](int y0) {
        if (tid < kPrYT) cstl[tid] = y0 + tid < C ? a.cst[y0 + tid] : -INFINITY;
      },
      ap::EveryBlock(),
      [&](int y0, int yb, const f32x4(&acc)[4]) {
        const float4 cv = *(const float4*)(cstl + yb * 16 + 4 * g);
        const float cr[4] = {cv.x, cv.y, cv.z, cv.w};
        const int cb = y0 + yb * 16 + 4 * g;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          float l[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            l[r] = cr[r] + acc[t][r];
            if (cb + r == yv[t]) ly[t] = l[r];
          }
          float b = m[t];
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (l[r] > b) b = l[r], bc[t] = cb + r;
          if (b > m[t]) s[t] = s[t] * expf(m[t] - b), m[t] = b;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (l[r] != -INFINITY) s[t] = s[t] + expf(l[r] - m[t]);
        }
      });

  // ---- the four lanes of a row, in lane order: every lane of the row computes the same
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    float ma[4], sa[4], la[4];
    int ka[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      ma[q] = __shfl(m[t], i + 16 * q, 64);
      sa[q] = __shfl(s[t], i + 16 * q, 64);
      ka[q] = __shfl(bc[t], i + 16 * q, 64);
      la[q] = __shfl(ly[t], i + 16 * q, 64);
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
      const float lse = M + logf(S);
      a.lse[row] = lse;
      a.pred[row] = kk;
      float v = 0.f;
      if (yv[t] >= 0) {  // class y belongs to the lane of group y / 4
        const int q = (yv[t] >> 2) & 3;
        const float lyv = q == 0 ? la[0] : (q == 1 ? la[1] : (q == 2 ? la[2] : la[3]));
        v = lse - lyv;
      }
      a.nll[row] = v;
    }
  }
}

template <int W>
int probe_rows_launch(const ProbeArgs& a, hipStream_t st) {
  const int smem = kPrYT * W * 4 + kPrYT * 4;
  hipLaunchKernelGGL((probe_rows_kernel<W>), dim3((unsigned)fh_cdiv(a.N, 256)), dim3(256), (size_t)smem, st, a);
  return fh_launch_status();
}

inline int64_t probe_slices(int64_t N) { return fh_cdiv(N, kPrSlice); }
inline int64_t probe_part_bytes(int64_t N, int64_t C, int64_t W) { return fh_cdiv(probe_slices(N) * C * (W + 1) * 4, 256) * 256; }
inline int64_t probe_ws(int64_t N, int64_t C, int64_t W) { return probe_part_bytes(N, C, W) + fh_cdiv(probe_slices(N) * 3 * 8, 256) * 256; }

// the totals, level one: a wave per slice, in the header's order -> tpart (slices, 3) float64
__global__ __launch_bounds__(256) void probe_slice_totals_kernel(const float* __restrict__ nll, const int32_t* __restrict__ y,
                                                                 const int32_t* __restrict__ pred, int N, int C, int64_t slices,
                                                                 double* __restrict__ tpart) {
  const int lane = threadIdx.x & 63;
  const int64_t slice = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slice >= slices) return;  // (uniform over the wave)
  const int64_t n0 = slice * kPrSlice;
  double sn = 0.0, sl = 0.0, sc = 0.0;
  for (int k = 0; k < kPrSlice / 64; ++k) {
    const int64_t row = n0 + lane + 64 * k;
    if (row < N) {
      const int v = y[row];
      const bool lab = (unsigned)v < (unsigned)C;
      sn += (double)nll[row];
      sl += lab ? 1.0 : 0.0;
      sc += (lab && pred[row] == v) ? 1.0 : 0.0;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sn += __shfl_xor(sn, o, 64);
    sl += __shfl_xor(sl, o, 64);
    sc += __shfl_xor(sc, o, 64);
  }
  if (lane == 0) tpart[slice * 3 + 0] = sn, tpart[slice * 3 + 1] = sl, tpart[slice * 3 + 2] = sc;
}

// level two: thread e of one wave adds total e over the slices in increasing order
__global__ void probe_totals_kernel(const double* __restrict__ tpart, int64_t slices, double* __restrict__ totals) {
  const int e = threadIdx.x;
  if (e >= 3) return;
  double v = 0.0;
  for (int64_t s = 0; s < slices; ++s) v += tpart[s * 3 + e];
  totals[e] = v;
}

// ---- pass 2
// T tiles of 16 classes per wave: the stationary fragments take T W / 4 registers, the accumulators 4 T (W / 16 + 1)
template <int W>
constexpr int probe_max_t() {
  return W <= 64 ? 4 : 2;
}

template <int W, int T>
__global__ __launch_bounds__(256) void probe_grad_kernel(ProbeArgs a) {
  constexpr int NJ = W / 16, CHN = W / 4, LOADS = kPrYT * CHN / 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ytile = smem;                            // [64][W] f32, swizzled
  float* lsel = (float*)(smem + kPrYT * W * 4);  // [64]: the rows' lse (0 for an unlabelled row)
  int* yl = (int*)(lsel + kPrYT);                // [64]: the rows' class, -1 for an unlabelled row

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i = lane & 15;
  const int C = a.C;
  const int c0 = (int)blockIdx.y * (64 * T) + wave * (16 * T);
  const bool active = c0 < C;  // (uniform over the wave: it still moves tiles and meets the barriers)
  const int64_t slice = blockIdx.x;
  const int n0 = (int)(slice * kPrSlice);  // (N <= 2^30: no overflow)
  const int n1 = n0 + kPrSlice < a.N ? n0 + kPrSlice : a.N;

  // the stationary fragments of the wave's classes (the layout of ap::load_stationary); classes past C: zeros and cst = -inf
  uint4 xf[T][NJ];
  float cstv[T];
  int cls[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int c = c0 + t * 16 + i;
    cls[t] = c;
    cstv[t] = c < C ? a.cst[c] : -INFINITY;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
      uint4 u = make_uint4(0, 0, 0, 0);
      if (c < C) u = *(const uint4*)(a.tab + (int64_t)c * a.ldt + 4 * g + 16 * jj);
      xf[t][jj] = u;
    }
  }
  f32x4 gacc[T][NJ + 1];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int dj = 0; dj <= NJ; ++dj) gacc[t][dj] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the loop of ap::stream, spelled out: pair() needs the tile in LDS a second time, and T is not always 4
  uint4 st[LOADS];
  auto issue = [&](int y0) {
#pragma unroll
    for (int p = 0; p < LOADS; ++p) {
      const int id = tid + p * 256;
      const int row = id / CHN, ch = id % CHN;
      st[p] = (y0 + row < n1) ? *(const uint4*)(a.x + (int64_t)(y0 + row) * a.ldx + ch * 4) : make_uint4(0, 0, 0, 0);
    }
  };
  issue(n0);
  for (int y0 = n0; y0 < n1; y0 += kPrYT) {
#pragma unroll
    for (int p = 0; p < LOADS; ++p) {
      const int id = tid + p * 256;
      *(uint4*)(ytile + ap::yoff<W>(id / CHN, id % CHN)) = st[p];
    }
    if (tid < kPrYT) {
      const int row = y0 + tid;
      int v = -1;
      float ls = 0.f;
      if (row < n1) {
        const int yy = a.y[row];
        if ((unsigned)yy < (unsigned)C) v = yy, ls = a.lse_in[row];
      }
      lsel[tid] = ls, yl[tid] = v;
    }
    __syncthreads();
    if (y0 + kPrYT < n1) issue(y0 + kPrYT);
    if (active) {
#pragma unroll 1
      for (int yb = 0; yb < kPrYT / 16; ++yb) {
        if (y0 + yb * 16 >= n1) break;
        uint4 af[NJ];
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) af[jj] = *(const uint4*)(ytile + ap::yoff<W>(yb * 16 + i, g + 4 * jj));
        f32x4 acc[T];
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
          const uint4 ua = af[jj];
#pragma unroll
          for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ua.x), __uint_as_float(xf[t][jj].x), acc[t], 0, 0, 0);
#pragma unroll
          for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ua.y), __uint_as_float(xf[t][jj].y), acc[t], 0, 0, 0);
#pragma unroll
          for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ua.z), __uint_as_float(xf[t][jj].z), acc[t], 0, 0, 0);
#pragma unroll
          for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ua.w), __uint_as_float(xf[t][jj].w), acc[t], 0, 0, 0);
        }
        // acc[t][r] = dot(class c0 + 16 t + i, row y0 + 16 yb + 4 g + r)
        const float4 lv = *(const float4*)(lsel + yb * 16 + 4 * g);
        const int4 yv = *(const int4*)(yl + yb * 16 + 4 * g);
        const float lsr[4] = {lv.x, lv.y, lv.z, lv.w};
        const int yr[4] = {yv.x, yv.y, yv.z, yv.w};
        float w[T][4];
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float l = cstv[t] + acc[t][r];
            const float p = expf(l - lsr[r]);
            const float res = p - (cls[t] == yr[r] ? 1.f : 0.f);
            w[t][r] = yr[r] >= 0 ? res : 0.f;
          }
        // G^T[d][c] += sum_rows x[row][d] * w[row][c]: A = x^T from LDS (lane: d = 16 dj + i, row = 4 g + r), B = w[t][r]
#pragma unroll
        for (int dj = 0; dj < NJ; ++dj) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = yb * 16 + 4 * g + r, d = dj * 16 + i;
            float av = *(const float*)(ytile + ap::yoff<W>(row, d >> 2) + (d & 3) * 4);
            av = yr[r] >= 0 ? av : 0.f;
#pragma unroll
            for (int t = 0; t < T; ++t) gacc[t][dj] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w[t][r], gacc[t][dj], 0, 0, 0);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int t = 0; t < T; ++t) gacc[t][NJ] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.f, w[t][r], gacc[t][NJ], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  if (!active) return;
  // gacc[t][dj][r] is (column 16 dj + 4 g + r, class c0 + 16 t + i); the bias product has the same sum in all of its sixteen rows
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (cls[t] >= C) continue;
    float* dst = a.part + (slice * C + cls[t]) * (W + 1);
#pragma unroll
    for (int dj = 0; dj < NJ; ++dj)
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[16 * dj + 4 * g + r] = gacc[t][dj][r];
    if (g == 0) dst[W] = gacc[t][NJ][0];
  }
}

template <int W, int T>
int probe_grad_launch_t(const ProbeArgs& a, hipStream_t st) {
  const int smem = kPrYT * W * 4 + kPrYT * 8;
  const dim3 grid((unsigned)probe_slices(a.N), (unsigned)fh_cdiv(a.C, 64 * T));
  hipLaunchKernelGGL((probe_grad_kernel<W, T>), grid, dim3(256), (size_t)smem, st, a);
  return fh_launch_status();
}

// the fewest tiles per wave with which one workgroup covers C, at most what W leaves registers for
template <int W>
int probe_grad_launch(const ProbeArgs& a, hipStream_t st) {
  constexpr int TM = probe_max_t<W>();
  if (a.C <= 64) return probe_grad_launch_t<W, 1>(a, st);
  if (a.C <= 128 || TM == 2) return probe_grad_launch_t<W, 2>(a, st);
  return probe_grad_launch_t<W, TM>(a, st);
}

// one thread per (c, column): the partials in slice order in float64
__global__ void probe_combine_kernel(const float* __restrict__ part, int64_t slices, int64_t total, double* __restrict__ grad) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  double v = 0.0;
  // the additions are one chain in slice order; the loads of kPrBatch slices fly together ahead of it
  const float* src = part + e;
  int64_t sl = 0;
  for (; sl + kPrBatch <= slices; sl += kPrBatch) {
    float p[kPrBatch];
#pragma unroll
    for (int j = 0; j < kPrBatch; ++j) p[j] = src[(sl + j) * total];
#pragma unroll
    for (int j = 0; j < kPrBatch; ++j) v += (double)p[j];
  }
  for (; sl < slices; ++sl) v += (double)src[sl * total];
  grad[e] = v;
}

// a (rows, width) f32 matrix: after the shapes of every argument, before the limits
inline bool probe_misaligned(const void* p, int64_t ld) { return ld % 4 != 0 || ((uintptr_t)p & 15) != 0; }
inline bool probe_bad_w(int64_t W) { return W < 16 || W > FHVAE_PROBE_MAX_W || W % 16 != 0; }

int probe_check(const float* x, int64_t ldx, int64_t N, int64_t W, const float* tab, int64_t ldt, const float* cst, int64_t C,
                const int32_t* y, const void* ws) {
  FH_CHECK_PTR(x);
  FH_CHECK_PTR(tab);
  FH_CHECK_PTR(cst);
  FH_CHECK_PTR(y);
  FH_CHECK_PTR(ws);
  FH_CHECK_POS(N);
  FH_CHECK_POS(C);
  if (probe_bad_w(W)) return FHVAE_ERR_SHAPE;
  if (ldx < W || ldt < W) return FHVAE_ERR_SHAPE;
  if (probe_misaligned(x, ldx) || probe_misaligned(tab, ldt) || ((uintptr_t)cst & 3) != 0 || ((uintptr_t)y & 3) != 0 ||
      ((uintptr_t)ws & 15) != 0)
    return FHVAE_ERR_ALIGN;
  return FHVAE_OK;
}

inline int probe_check_limits(int64_t N, int64_t C) {
  return (N > FHVAE_PROBE_MAX_ROWS || C > FHVAE_PROBE_MAX_CLASSES) ? FHVAE_ERR_LIMIT : FHVAE_OK;
}

}  // namespace

}  // namespace fh

using namespace fh;

extern "C" int64_t fhvae_probe_ws_bytes(int64_t N, int64_t C, int64_t W) {
  if (N < 1 || C < 1 || N > FHVAE_PROBE_MAX_ROWS || C > FHVAE_PROBE_MAX_CLASSES || probe_bad_w(W)) return 0;
  return probe_ws(N, C, W);
}

extern "C" int fhvae_probe_rows(const float* x, int64_t ldx, int64_t N, int64_t W, const float* tab, int64_t ldt, const float* cst,
                                int64_t C, const int32_t* y, float* lse, int32_t* pred, float* nll, double* totals, void* ws,
                                int64_t ws_bytes, void* stream) {
  FH_CHECK_PTR(lse);
  FH_CHECK_PTR(pred);
  FH_CHECK_PTR(nll);
  FH_CHECK_PTR(totals);
  int rc = probe_check(x, ldx, N, W, tab, ldt, cst, C, y, ws);
  if (rc != FHVAE_OK) return rc;
  if (((uintptr_t)lse & 3) != 0 || ((uintptr_t)pred & 3) != 0 || ((uintptr_t)nll & 3) != 0 || ((uintptr_t)totals & 7) != 0)
    return FHVAE_ERR_ALIGN;
  rc = probe_check_limits(N, C);
  if (rc != FHVAE_OK) return rc;
  if (ws_bytes < probe_ws(N, C, W)) return FHVAE_ERR_SHAPE;
  ProbeArgs a = {};
  a.x = x, a.tab = tab, a.cst = cst, a.y = y, a.lse = lse, a.pred = pred, a.nll = nll;
  a.ldx = ldx, a.ldt = ldt, a.N = (int)N, a.C = (int)C;
  hipStream_t st = (hipStream_t)stream;
  rc = fh_allpairs_dispatch(W, [&](auto w) { return probe_rows_launch<decltype(w)::value>(a, st); });
  if (rc != FHVAE_OK) return rc;
  const int64_t slices = probe_slices(N);
  double* tpart = (double*)((char*)ws + probe_part_bytes(N, C, W));
  hipLaunchKernelGGL(probe_slice_totals_kernel, dim3((unsigned)fh_cdiv(slices, 4)), dim3(256), 0, st, nll, y, pred, (int)N, (int)C, slices,
                     tpart);
  rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  hipLaunchKernelGGL(probe_totals_kernel, dim3(1), dim3(64), 0, st, tpart, slices, totals);
  return fh_launch_status();
}

extern "C" int fhvae_probe_grad(const float* x, int64_t ldx, int64_t N, int64_t W, const float* tab, int64_t ldt, const float* cst,
                                int64_t C, const int32_t* y, const float* lse, double* grad, void* ws, int64_t ws_bytes,
                                void* stream) {
  FH_CHECK_PTR(lse);
  FH_CHECK_PTR(grad);
  int rc = probe_check(x, ldx, N, W, tab, ldt, cst, C, y, ws);
  if (rc != FHVAE_OK) return rc;
  if (((uintptr_t)lse & 3) != 0 || ((uintptr_t)grad & 7) != 0) return FHVAE_ERR_ALIGN;
  rc = probe_check_limits(N, C);
  if (rc != FHVAE_OK) return rc;
  if (ws_bytes < probe_ws(N, C, W)) return FHVAE_ERR_SHAPE;
  ProbeArgs a = {};
  a.x = x, a.tab = tab, a.cst = cst, a.y = y, a.lse_in = lse, a.part = (float*)ws;
  a.ldx = ldx, a.ldt = ldt, a.N = (int)N, a.C = (int)C;
  hipStream_t st = (hipStream_t)stream;
  rc = fh_allpairs_dispatch(W, [&](auto w) { return probe_grad_launch<decltype(w)::value>(a, st); });
  if (rc != FHVAE_OK) return rc;
  const int64_t total = C * (W + 1);
  hipLaunchKernelGGL(probe_combine_kernel, dim3((unsigned)fh_cdiv(total, 256)), dim3(256), 0, st, a.part, probe_slices(N), total, grad);
  return fh_launch_status();
}
