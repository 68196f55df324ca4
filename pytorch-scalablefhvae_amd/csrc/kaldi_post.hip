// kaldi_post.hip -- cepstra, delta features and sliding-window CMVN (include/fhvae_kaldi_post.h):
//   fhvae_kaldi_cepstra      : out = lifter * (dct . log-mel row), C0 optionally replaced by a floored energy;
//   fhvae_kaldi_add_deltas   : [x, delta x, delta delta x] of every row, the edges replicated inside the utterance;
//   fhvae_kaldi_cmvn_sliding : every row less the mean of its window (and over the window's standard deviation).
//
// Cepstra.  A workgroup takes kCepRows consecutive rows.  The DCT matrix and the rows are staged in LDS with an odd row
// stride (lanes that differ in k read different banks; lanes that share rows read one address).  A thread owns one
// coefficient k of four rows (row r * 16 + g of the tile, r < 4): one read of dct[k][j] feeds four fused multiply-adds, and
// for fixed r the lanes' stores are consecutive floats of `out`.  The chain over j runs from 0 upwards, per row.
//
// Deltas.  A workgroup takes kDelRows consecutive rows of the batch and all D columns.  One thread per row finds the row's
// utterance (binary search in frame_ptr) and leaves its bounds in LDS; then one thread per (row, column), the column the
// fast index, walks the taps straight from global memory: a row is read by the 1 + (2w+1) + (4w+1) taps of its neighbours,
// which are in the same or the next workgroup, so all but the first read come from the caches.  (Not measured against
// staging the tile and its halo in LDS.)
//
// Sliding CMVN.  Utterance u owns the slots frame_ptr[u] / C + 2 u + k, k <= ceil(T_u / C), of two arrays of float64 pairs
// (sum, sum of squares) per column (C = FHVAE_KPOST_CHUNK; distinct utterances get distinct slots because
// floor(a / C) + ceil(T / C) + 1 <= floor((a + T) / C) + 2, and there are at most n / C + 2 U of them):
//   totals : one wave per slot, a thread per column adds the chunk's rows in row order            -> tot
//   scan   : one thread per (utterance, column) adds the utterance's chunk totals in chunk order  -> pre (exclusive, with the
//            grand total as the last entry)
//   apply  : one workgroup per (slot, group of kCmvnCols columns): thread i owns frame i of the chunk and computes its window
//            [b, e).  b and e each rise by at most one per frame, so the b of a tile lie in at most two chunks, and so do
//            the e.  All threads stage the rows of those chunks in LDS; one thread per (end, chunk, column) re-scans its
//            chunk there in row order and leaves S(x) = pre + Q for the x the tile needs (at most C values per end); then
//            every thread forms its sums as S(e) - S(b).  (Re-scanning straight from global memory took 1.65 ms for an
//            hour of 39 columns, against 0.78 ms from LDS.)
//            A per-frame prefix is never stored, and an hour-long utterance is spread over as many workgroups as it has
//            chunks.
// The tile sizes above are first choices, none of them is measured against another.
//
// Pointer errors: a check kernel validates frame_ptr and sets FHVAE_KPOST_BAD_PTR; the kernels behind it then write nothing.
// They also re-check the utterance of every row they touch, so no input makes them read or write out of bounds.
#pragma clang fp contract(off)

#include "common.h"

#include "../../include/fhvae_kaldi_post.h"

namespace fh {

constexpr int kKpThreads = 256;
constexpr int kCepRows = 64;                     // rows per workgroup of the cepstra kernel: 4 per thread, 16 row groups
constexpr int kDelRows = 64;                     // rows per workgroup of the delta kernel
constexpr int kDelMaxScales = 1 + (2 * FHVAE_KPOST_MAX_WINDOW + 1) + (4 * FHVAE_KPOST_MAX_WINDOW + 1);
constexpr int kCmvnCols = 4;                     // columns per workgroup of the CMVN's apply kernel (32 KB of LDS)
constexpr int kCmvnCap = FHVAE_KPOST_CHUNK;      // S values per window end a tile can need

static_assert(FHVAE_KPOST_CHUNK == kKpThreads, "one thread per frame of a chunk");
static_assert(kCepRows == 4 * 16, "four rows per thread in 16 row groups");

// the last u in [0, U) with ptr[u] <= x (0 when there is none); reads ptr[0 .. U - 1] only.  With empty utterances in the
// batch this is the one that holds row x: ptr[u + 1] > x.
__device__ __forceinline__ int64_t kp_find(const int64_t* __restrict__ ptr, int64_t U, int64_t x) {
  int64_t lo = 0, hi = U - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (ptr[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// one thread per utterance: frame_ptr starts at 0, ends at n and does not decrease
__global__ void kp_check_kernel(const int64_t* __restrict__ frame_ptr, int64_t U, int64_t n, int32_t* status) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const int64_t f0 = frame_ptr[u], f1 = frame_ptr[u + 1];
  bool ok = f0 >= 0 && f1 <= n && f1 >= f0;
  if (u == 0) ok = ok && f0 == 0;
  if (u == U - 1) ok = ok && f1 == n;
  if (!ok) atomicOr(status, FHVAE_KPOST_BAD_PTR);
}

// --------------------------------------------------------------------------------------------------------------- cepstra
__global__ void __launch_bounds__(kKpThreads) kp_cepstra_kernel(const float* __restrict__ logmel, int64_t ld, int64_t n, int B,
                                                                const float* __restrict__ dct, int C,
                                                                const float* __restrict__ lifter, const float* __restrict__ energy,
                                                                float floor_e, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float kp_sm[];
  const int tid = threadIdx.x, Bp = B | 1;
  float* ds = kp_sm;            // (C, Bp)
  float* xs = kp_sm + C * Bp;   // (kCepRows, Bp)
  const int64_t f0 = (int64_t)blockIdx.x * kCepRows;
  for (int i = tid; i < C * B; i += kKpThreads) ds[(i / B) * Bp + i % B] = dct[i];
  for (int i = tid; i < kCepRows * B; i += kKpThreads) {
    const int r = i / B, j = i % B;
    xs[r * Bp + j] = f0 + r < n ? logmel[(f0 + r) * ld + j] : 0.f;
  }
  __syncthreads();
  for (int it = tid; it < C * 16; it += kKpThreads) {
    const int g = it / C, k = it % C;
    const float* w = ds + k * Bp;
    const float* x = xs + g * Bp;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < B; ++j) {
      const float wj = w[j];
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = fmaf(wj, x[r * 16 * Bp + j], acc[r]);
    }
    const float lf = lifter != nullptr ? lifter[k] : 1.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t f = f0 + r * 16 + g;
      if (f < n) {
        float v = lifter != nullptr ? lf * acc[r] : acc[r];
        if (k == 0 && energy != nullptr) {
          const float e = energy[f];
          v = e > floor_e ? e : floor_e;
        }
        out[f * C + k] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- deltas
__global__ void __launch_bounds__(kKpThreads) kp_deltas_kernel(const float* __restrict__ in, const int64_t* __restrict__ frame_ptr,
                                                               int64_t U, int64_t n, int D, int order, int window,
                                                               const float* __restrict__ scales, float* __restrict__ out,
                                                               const int32_t* status) {
  __shared__ float sc[kDelMaxScales];
  __shared__ int64_t ua[kDelRows], ue[kDelRows];
  if (*status & FHVAE_KPOST_BAD_PTR) return;  // (set by the check kernel)
  const int tid = threadIdx.x;
  const int64_t g0 = (int64_t)blockIdx.x * kDelRows;
  const int ns = 1 + (2 * window + 1) + (order == 2 ? 4 * window + 1 : 0);
  if (tid < ns && tid < kDelMaxScales) sc[tid] = scales[tid];
  if (tid < kDelRows) {
    const int64_t g = g0 + tid;
    int64_t a = 0, e = 0;  // (e = 0: no row)
    if (g < n) {
      const int64_t u = kp_find(frame_ptr, U, g);
      a = frame_ptr[u], e = frame_ptr[u + 1];
      if (!(a >= 0 && a <= g && g < e && e <= n)) a = 0, e = 0;
    }
    ua[tid] = a, ue[tid] = e;
  }
  __syncthreads();
  const int OD = (order + 1) * D;
  for (int i = tid; i < kDelRows * D; i += kKpThreads) {
    const int r = i / D, d = i % D;
    const int64_t a = ua[r], e = ue[r];
    if (e == 0) continue;
    const int64_t g = g0 + r, t = g - a, T = e - a;
    float* o = out + g * OD + d;
    o[0] = in[g * D + d];
    int off = 1;
    for (int k = 1; k <= order; ++k) {
      const int hw = k * window;
      float acc = 0.f;
      for (int m = 0; m <= 2 * hw; ++m) {
        int64_t tt = t + m - hw;
        tt = tt < 0 ? 0 : (tt > T - 1 ? T - 1 : tt);
        acc = fmaf(sc[off + m], in[(a + tt) * D + d], acc);
      }
      o[(int64_t)k * D] = acc;
      off += 2 * hw + 1;
    }
  }
}

// ----------------------------------------------------------------------------------------------------------- sliding CMVN
struct KpWs {  // the workspace of fhvae_kaldi_cmvn_sliding: (slots, D, 2) float64 each
  int64_t slots;
  double* tot;  // the chunk totals
  double* pre;  // their exclusive prefix inside the utterance, the grand total last
};

__host__ __device__ inline int64_t kp_slots(int64_t n, int64_t U) { return n / FHVAE_KPOST_CHUNK + 2 * U; }
__device__ __forceinline__ int64_t kp_key(int64_t a, int64_t u) { return a / FHVAE_KPOST_CHUNK + 2 * u; }

// the utterance that owns slot b -> its bounds and the chunk index k (k == chunks: the grand-total entry); false: none
__device__ __forceinline__ bool kp_slot_owner(const int64_t* __restrict__ frame_ptr, int64_t U, int64_t n, int64_t b, int64_t* a_,
                                              int64_t* e_, int64_t* k_, int64_t* s0_) {
  int64_t lo = 0, hi = U - 1;  // the last u with key(u) <= b (the key rises strictly with u for a checked frame_ptr)
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    const int64_t am = frame_ptr[mid];
    if (am >= 0 && kp_key(am, mid) <= b) lo = mid; else hi = mid - 1;
  }
  const int64_t a = frame_ptr[lo], e = frame_ptr[lo + 1];
  if (!(a >= 0 && e <= n && e >= a)) return false;
  const int64_t k = b - kp_key(a, lo);
  if (k < 0 || k > (e - a + FHVAE_KPOST_CHUNK - 1) / FHVAE_KPOST_CHUNK) return false;
  *a_ = a, *e_ = e, *k_ = k, *s0_ = kp_key(a, lo);
  return true;
}

// one wave per slot, a thread per column: the chunk's rows in row order
__global__ void __launch_bounds__(64) kp_cmvn_totals_kernel(const float* __restrict__ in, const int64_t* __restrict__ frame_ptr,
                                                            int64_t U, int64_t n, int D, double* __restrict__ tot,
                                                            const int32_t* status) {
  if (*status & FHVAE_KPOST_BAD_PTR) return;
  const int64_t b = blockIdx.x;
  int64_t a, e, k, s0;
  if (!kp_slot_owner(frame_ptr, U, n, b, &a, &e, &k, &s0)) return;
  const int64_t c0 = a + k * FHVAE_KPOST_CHUNK;
  if (c0 >= e) return;  // (the grand-total entry, or a slot no utterance owns)
  const int len = (int)(e - c0 < FHVAE_KPOST_CHUNK ? e - c0 : FHVAE_KPOST_CHUNK);
  for (int d = threadIdx.x; d < D; d += 64) {
    const float* p = in + c0 * D + d;
    double s = 0.0, s2 = 0.0;
#pragma unroll 8
    for (int r = 0; r < len; ++r) {
      const double v = (double)p[(int64_t)r * D];
      s = s + v;
      s2 = s2 + v * v;
    }
    tot[(b * D + d) * 2] = s;
    tot[(b * D + d) * 2 + 1] = s2;
  }
}

// one thread per (utterance, column): the chunk totals in chunk order
__global__ void __launch_bounds__(kKpThreads) kp_cmvn_scan_kernel(const int64_t* __restrict__ frame_ptr, int64_t U, int64_t n, int D,
                                                                  int64_t slots, const double* __restrict__ tot,
                                                                  double* __restrict__ pre, const int32_t* status) {
  if (*status & FHVAE_KPOST_BAD_PTR) return;
  const int64_t i = (int64_t)blockIdx.x * kKpThreads + threadIdx.x;
  if (i >= U * D) return;
  const int64_t u = i / D;
  const int d = (int)(i % D);
  const int64_t a = frame_ptr[u], e = frame_ptr[u + 1];
  if (!(a >= 0 && e <= n && e >= a)) return;
  const int64_t s0 = kp_key(a, u), chunks = (e - a + FHVAE_KPOST_CHUNK - 1) / FHVAE_KPOST_CHUNK;
  double s = 0.0, s2 = 0.0;
  for (int64_t k = 0; k <= chunks && s0 + k < slots; ++k) {
    const int64_t j = ((s0 + k) * D + d) * 2;
    pre[j] = s;
    pre[j + 1] = s2;
    if (k < chunks) {
      s = s + tot[j];
      s2 = s2 + tot[j + 1];
    }
  }
}

// the window [b, e) of frame t of T (include/fhvae_kaldi_post.h)
__host__ __device__ inline void kp_window(int64_t t, int64_t T, int64_t cmn_window, int64_t min_window, int center, int64_t* b_,
                                          int64_t* e_) {
  int64_t b, e;
  if (center) {
    b = t - cmn_window / 2;
    e = b + cmn_window;
  } else {
    b = t - cmn_window;
    e = t + 1;
  }
  if (b < 0) {
    e -= b;
    b = 0;
  }
  if (!center && e > t) e = t + 1 > min_window ? t + 1 : min_window;
  if (e > T) {
    b -= e - T;
    e = T;
    if (b < 0) b = 0;
  }
  *b_ = b, *e_ = e;
}

__global__ void __launch_bounds__(kKpThreads) kp_cmvn_apply_kernel(const float* __restrict__ in, const int64_t* __restrict__ frame_ptr,
                                                                   int64_t U, int64_t n, int D, int64_t cmn_window,
                                                                   int64_t min_window, int center, int norm_vars, int64_t slots,
                                                                   const double* __restrict__ pre, float* __restrict__ out,
                                                                   const int32_t* status) {
  __shared__ double ps[2][kCmvnCols][2][kCmvnCap];  // [end: b, e][column][sum, squares][x - the end's smallest x]
  __shared__ float xr[2][2][FHVAE_KPOST_CHUNK][kCmvnCols];  // [end][chunk of the two][row][column]: the rows to re-scan
  __shared__ int64_t wl[kKpThreads / 64][4];         // per wave: the smallest and largest b, the smallest and largest e
  if (*status & FHVAE_KPOST_BAD_PTR) return;
  const int tid = threadIdx.x;
  int64_t a, e, k, s0;
  // (everything up to the barriers is the same in all threads: they are reached by all or none)
  if (!kp_slot_owner(frame_ptr, U, n, blockIdx.x, &a, &e, &k, &s0)) return;
  const int64_t T = e - a, t0 = k * FHVAE_KPOST_CHUNK;
  if (t0 >= T) return;
  const int nf = (int)(T - t0 < FHVAE_KPOST_CHUNK ? T - t0 : FHVAE_KPOST_CHUNK);
  const int64_t t = t0 + tid;
  int64_t b_ = 0, e_ = 0;
  if (tid < nf) kp_window(t, T, cmn_window, min_window, center, &b_, &e_);
  const bool has = tid < nf && 0 <= b_ && b_ < e_ && e_ <= T;  // (true for every frame: the rule gives 0 <= b < e <= T)
  {
    const int64_t big = INT64_MAX;
    int64_t v[4] = {has ? b_ : big, has ? b_ : -1, has ? e_ : big, has ? e_ : -1};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t w = __shfl_xor((long long)v[q], o, 64);
        v[q] = (q & 1) ? (w > v[q] ? w : v[q]) : (w < v[q] ? w : v[q]);
      }
    }
    if ((tid & 63) == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) wl[tid >> 6][q] = v[q];
    }
  }
  __syncthreads();
  int64_t lim[4];  // the smallest and largest b, the smallest and largest e of the tile
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    int64_t v = wl[0][q];
#pragma unroll
    for (int w = 1; w < kKpThreads / 64; ++w) v = (q & 1) ? (wl[w][q] > v ? wl[w][q] : v) : (wl[w][q] < v ? wl[w][q] : v);
    lim[q] = v;
  }
  // the rows of the (at most) two chunks the b of the tile lie in, and of the two the e lie in: all threads, 16-byte segments
  for (int i = tid; i < 4 * FHVAE_KPOST_CHUNK * kCmvnCols; i += kKpThreads) {
    const int col = i % kCmvnCols, r = (i / kCmvnCols) % FHVAE_KPOST_CHUNK, ci = (i / (kCmvnCols * FHVAE_KPOST_CHUNK)) & 1,
              end = i / (2 * kCmvnCols * FHVAE_KPOST_CHUNK);
    const int d = blockIdx.y * kCmvnCols + col;
    const int64_t xmin = end ? lim[2] : lim[0], xmax = end ? lim[3] : lim[1];  // (no indexed register array)
    const int64_t x = (xmin / FHVAE_KPOST_CHUNK + ci) * FHVAE_KPOST_CHUNK + r;
    float v = 0.f;
    if (d < D && xmin >= 0 && xmax <= T && x < xmax && x < T) v = in[(a + x) * D + d];  // (S(xmax) needs the rows below xmax)
    xr[end][ci][r][col] = v;
  }
  __syncthreads();
  if (tid < 4 * kCmvnCols) {  // one thread per (end, chunk of the two, column): the chunk's rows in row order
    const int col = tid % kCmvnCols, ci = (tid / kCmvnCols) & 1, end = tid / (2 * kCmvnCols);
    const int d = blockIdx.y * kCmvnCols + col;
    const int64_t xmin = end ? lim[2] : lim[0], xmax = end ? lim[3] : lim[1];  // (no indexed register array)
    const int64_t cc = xmin / FHVAE_KPOST_CHUNK + ci, base = cc * FHVAE_KPOST_CHUNK;
    if (d < D && xmin >= 0 && xmax <= T && base <= xmax && s0 + cc < slots) {
      const double P = pre[((s0 + cc) * D + d) * 2], P2 = pre[((s0 + cc) * D + d) * 2 + 1];
      const int rmax = (int)(xmax - base < FHVAE_KPOST_CHUNK - 1 ? xmax - base : FHVAE_KPOST_CHUNK - 1);
      double q = 0.0, q2 = 0.0;
      for (int r = 0; r <= rmax; ++r) {
        const int64_t x = base + r;
        if (x >= xmin && x - xmin < kCmvnCap) {
          ps[end][col][0][x - xmin] = P + q;
          ps[end][col][1][x - xmin] = P2 + q2;
        }
        if (x < xmax) {  // (x < xmax <= T: a row of the utterance, staged above)
          const double v = (double)xr[end][ci][r][col];
          q = q + v;
          q2 = q2 + v * v;
        }
      }
    }
  }
  __syncthreads();
  if (!has) return;
  const int64_t ib = b_ - lim[0], ie = e_ - lim[2];
  if (ib >= kCmvnCap || ie >= kCmvnCap) return;  // (never: b and e rise by at most one per frame)
  const double N = (double)(e_ - b_);
#pragma unroll
  for (int col = 0; col < kCmvnCols; ++col) {
    const int d = blockIdx.y * kCmvnCols + col;
    if (d >= D) break;
    const double x = (double)in[(a + t) * D + d];
    const double mean = (ps[1][col][0][ie] - ps[0][col][0][ib]) / N;
    double y = x - mean;
    if (norm_vars) {
      double var = (ps[1][col][1][ie] - ps[0][col][1][ib]) / N - mean * mean;
      var = var > 1e-10 ? var : 1e-10;
      if (e_ - b_ == 1) var = 1.0;
      y = y * (1.0 / sqrt(var));
    }
    out[(a + t) * D + d] = (float)y;
  }
}

}  // namespace fh

using namespace fh;

extern "C" int fhvae_kaldi_cepstra(const float* logmel, int64_t ld, int64_t n, int64_t B, const float* dct, int64_t C,
                                   const float* lifter, const float* energy, float log_energy_floor, float* out, void* stream) {
  if (n < 0 || C < 1 || B < 1 || C > B || ld < B) return FHVAE_ERR_SHAPE;
  if (B > FHVAE_KPOST_MAX_BINS) return FHVAE_ERR_LIMIT;
  if (log_energy_floor != log_energy_floor) return FHVAE_ERR_SHAPE;  // (NaN)
  FH_CHECK_PTR(dct);
  if (n == 0) return FHVAE_OK;
  FH_CHECK_PTR(logmel);
  FH_CHECK_PTR(out);
  const int64_t blocks = fh_cdiv(n, kCepRows);
  FH_CHECK_I32(blocks);
  const int smem = (int)((C + kCepRows) * (B | 1) * sizeof(float));  // at most 97 KB
  if (smem > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kp_cepstra_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kp_cepstra_kernel, dim3((unsigned)blocks), dim3(kKpThreads), (size_t)smem, (hipStream_t)stream, logmel, ld, n,
                     (int)B, dct, (int)C, lifter, energy, log_energy_floor, out);
  return fh_launch_status();
}

extern "C" int fhvae_kaldi_add_deltas(const float* in, const int64_t* frame_ptr, int64_t U, int64_t n, int64_t D, int64_t order,
                                      int64_t window, const float* scales, float* out, int32_t* status, void* stream) {
  FH_CHECK_PTR(frame_ptr);
  FH_CHECK_PTR(scales);
  FH_CHECK_PTR(status);
  if (n < 0 || D < 1 || order < 1 || order > 2 || window < 1) return FHVAE_ERR_SHAPE;
  if (window > FHVAE_KPOST_MAX_WINDOW || (order + 1) * D > FHVAE_KPOST_MAX_COLS) return FHVAE_ERR_LIMIT;
  if (n == 0) return FHVAE_OK;
  FH_CHECK_PTR(in);
  FH_CHECK_PTR(out);
  FH_CHECK_POS(U);
  const int64_t blocks = fh_cdiv(n, kDelRows), ublocks = fh_cdiv(U, kKpThreads);
  FH_CHECK_I32(blocks);
  FH_CHECK_I32(ublocks);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(kp_check_kernel, dim3((unsigned)ublocks), dim3(kKpThreads), 0, st, frame_ptr, U, n, status);
  hipLaunchKernelGGL(kp_deltas_kernel, dim3((unsigned)blocks), dim3(kKpThreads), 0, st, in, frame_ptr, U, n, (int)D, (int)order,
                     (int)window, scales, out, status);
  return fh_launch_status();
}

extern "C" int64_t fhvae_kaldi_post_ws_bytes(int64_t n, int64_t U, int64_t D) {
  if (n < 0 || U < 0 || D < 1) return FHVAE_ERR_SHAPE;
  if (D > FHVAE_KPOST_MAX_COLS) return FHVAE_ERR_LIMIT;
  return 2 * kp_slots(n, U) * D * 2 * (int64_t)sizeof(double);
}

extern "C" int fhvae_kaldi_cmvn_sliding(const float* in, const int64_t* frame_ptr, int64_t U, int64_t n, int64_t D,
                                        int64_t cmn_window, int64_t min_window, int center, int norm_vars, void* ws, int64_t ws_bytes,
                                        float* out, int32_t* status, void* stream) {
  FH_CHECK_PTR(frame_ptr);
  FH_CHECK_PTR(status);
  if (n < 0 || D < 1 || cmn_window < 1 || min_window < 1) return FHVAE_ERR_SHAPE;
  if ((center != 0 && center != 1) || (norm_vars != 0 && norm_vars != 1)) return FHVAE_ERR_SHAPE;
  if (D > FHVAE_KPOST_MAX_COLS) return FHVAE_ERR_LIMIT;
  FH_CHECK_I32(cmn_window);
  FH_CHECK_I32(min_window);
  if (n == 0) return FHVAE_OK;
  FH_CHECK_PTR(in);
  FH_CHECK_PTR(ws);
  FH_CHECK_PTR(out);
  FH_CHECK_POS(U);
  if (in == out) return FHVAE_ERR_SHAPE;
  if (ws_bytes < fhvae_kaldi_post_ws_bytes(n, U, D)) return FHVAE_ERR_SHAPE;
  if (((uintptr_t)ws & 7) != 0) return FHVAE_ERR_ALIGN;
  KpWs w;
  w.slots = kp_slots(n, U);
  w.tot = (double*)ws;
  w.pre = w.tot + w.slots * D * 2;
  const int64_t ublocks = fh_cdiv(U, kKpThreads), sblocks = fh_cdiv(U * D, kKpThreads);
  FH_CHECK_I32(w.slots);
  FH_CHECK_I32(ublocks);
  FH_CHECK_I32(sblocks);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(kp_check_kernel, dim3((unsigned)ublocks), dim3(kKpThreads), 0, st, frame_ptr, U, n, status);
  hipLaunchKernelGGL(kp_cmvn_totals_kernel, dim3((unsigned)w.slots), dim3(64), 0, st, in, frame_ptr, U, n, (int)D, w.tot, status);
  hipLaunchKernelGGL(kp_cmvn_scan_kernel, dim3((unsigned)sblocks), dim3(kKpThreads), 0, st, frame_ptr, U, n, (int)D, w.slots, w.tot,
                     w.pre, status);
  hipLaunchKernelGGL(kp_cmvn_apply_kernel, dim3((unsigned)w.slots, (unsigned)fh_cdiv(D, kCmvnCols)), dim3(kKpThreads), 0, st, in,
                     frame_ptr, U, n, (int)D, cmn_window, min_window, center, norm_vars, w.slots, w.pre, out, status);
  return fh_launch_status();
}
