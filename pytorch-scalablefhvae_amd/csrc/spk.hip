// spk.hip -- the speaker back end on embeddings (include/fhvae_spk.h): the row transform of an LDA / PLDA model, and the PLDA
// log-likelihood ratio of all pairs of rows in one pass with no (S x S) temporary, or of a list of trials.
//
//   s(i, j) = (v_i . v_j + (a[i] + a[j])) + c          for every i < j with label[i] >= 0 and label[j] >= 0
//
// The contraction is allpairs_f32.h's pass over the upper triangle, tiled as sv.hip tiles it (256 stationary rows per
// workgroup, the streamed rows in chunks, the blocks below the diagonal skipped, tails with label -1).  ONE kernel template
// walks the tiles; its epilogue is a policy class:
//   RangeEpi   keeps per lane the smallest and the largest score of either class as order-preserving 32-bit keys, merges them
//              over the wave by shuffles and leaves them in the workspace with four vector atomic min / max per wave
//   HistEpi    turns a score into a bin (one subtraction, one product: no division) and counts it in a per-workgroup LDS
//              histogram (ds_add_u32), flushed with vector 64-bit global atomic adds as sv_hist_kernel does
// Both results are free of any order of arrival (a minimum in a total order, integer counts).
// What a trial's score is, is a second policy: LlrScore, the s above (the default), or NormScore, the normalised score of
// include/fhvae_snorm.h, sn = 0.5 ((s - mu_i) r_i + (s - mu_j) r_j), with mu and r of the stationary rows in registers and of
// the streamed rows beside ya / yl in LDS.
//
// Symmetry, bit for bit: the dot is symmetric (allpairs_f32.h, THE ORDER) and a[i] + a[j] commutes.
// The file is built with -ffp-contract=off (every f32 operation below is rounded once unless it is written fmaf) and with
// correctly rounded division and square root (fhvae_spk_project's normalisation).
#include <algorithm>
#include <cmath>

#include "allpairs_f32.h"

#include "../../include/fhvae_snorm.h"
#include "../../include/fhvae_spk.h"

namespace fh {

namespace {

constexpr int kSpkYT = ap::kYT;
constexpr int kSpkMinChunk = 512;     // streamed rows per workgroup, at least (sv.hip's: a workgroup zeroes and flushes 2 NB bins)
constexpr int kSpkWorkgroups = 8192;  // launched workgroups aimed at (about half of them lie below the diagonal and return)

// f32 -> a 32-bit key whose unsigned order is the order of the floats (-inf lowest, -0 below +0, +inf highest), and back
__host__ __device__ __forceinline__ unsigned spk_key(float f) {
  const unsigned b = __builtin_bit_cast(unsigned, f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ __forceinline__ float spk_unkey(unsigned k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

struct SpkArgs {
  const float* v;        // (S, D), leading dimension ld
  const float* a;        // (S)
  const int32_t* label;  // (S)
  int32_t* status;
  unsigned* keys;            // RangeEpi: [class][min, max]
  unsigned long long* hist;  // HistEpi: (2, NB)
  int64_t ld;
  float c, lo, scale;
  int S, NB, chunk;
  const float* mu;  // NormScore: (S)
  const float* r;   // NormScore: (S)
};

struct RangeEpi {
  static constexpr bool kHist = false;
  unsigned k[4];  // [class][min, max]
  __device__ __forceinline__ RangeEpi(const SpkArgs&, unsigned*) {
    k[0] = k[2] = 0xffffffffu;
    k[1] = k[3] = 0u;
  }
  __device__ __forceinline__ void trial(int cls, float s) {
    const unsigned key = spk_key(s);
    k[2 * cls] = min(k[2 * cls], key);
    k[2 * cls + 1] = max(k[2 * cls + 1], key);
  }
  __device__ __forceinline__ void finish(const SpkArgs& a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      k[0] = min(k[0], (unsigned)__shfl_xor((int)k[0], off, 64));
      k[1] = max(k[1], (unsigned)__shfl_xor((int)k[1], off, 64));
      k[2] = min(k[2], (unsigned)__shfl_xor((int)k[2], off, 64));
      k[3] = max(k[3], (unsigned)__shfl_xor((int)k[3], off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMin(a.keys + 0, k[0]);
      atomicMax(a.keys + 1, k[1]);
      atomicMin(a.keys + 2, k[2]);
      atomicMax(a.keys + 3, k[3]);
    }
  }
};

struct HistEpi {
  static constexpr bool kHist = true;
  unsigned* h;  // [2][NB] in LDS
  float lo, scale, top;
  int NB;
  __device__ __forceinline__ HistEpi(const SpkArgs& a, unsigned* lds) : h(lds), lo(a.lo), scale(a.scale), top((float)(a.NB - 1)), NB(a.NB) {
    for (int e = threadIdx.x; e < 2 * NB; e += 256) h[e] = 0u;  // (stream()'s first barrier stands between this and the first count)
  }
  __device__ __forceinline__ void trial(int cls, float s) {
    const float b = fminf(fmaxf(floorf((s - lo) * scale), 0.f), top);  // (fmaxf(NaN, 0) = 0)
    atomicAdd(&h[cls * NB + (int)b], 1u);
  }
  // a workgroup's count of a bin is below 2^32 (256 * chunk trials); the sum over workgroups is 64-bit.  (stream() ends on a barrier)
  __device__ __forceinline__ void finish(const SpkArgs& a) {
    for (int e = threadIdx.x; e < 2 * NB; e += 256) {
      const unsigned n = h[e];
      if (n) atomicAdd(a.hist + e, (unsigned long long)n);
    }
  }
};

// the plain score: nothing beside the tile, nothing in registers
struct LlrScore {
  static constexpr int kSide = 0;  // bytes of LDS per streamed row
  __device__ __forceinline__ LlrScore(const SpkArgs&, int, float*) {}
  __device__ __forceinline__ void side(const SpkArgs&, int, int, int) {}
  __device__ __forceinline__ void block(int, int) {}
  __device__ __forceinline__ float operator()(float s, int, int) const { return s; }
};

struct NormScore {
  static constexpr int kSide = 8;
  float xmu[4], xr[4], ymur[4], yrr[4];
  float *ymu, *yr;  // [YT] each
  __device__ __forceinline__ NormScore(const SpkArgs& a, int x0, float* lds) : ymu(lds), yr(lds + kSpkYT) {
    const int i = threadIdx.x & 15;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int x = x0 + t * 16 + i;
      xmu[t] = x < a.S ? a.mu[x] : 0.f;
      xr[t] = x < a.S ? a.r[x] : 0.f;
    }
  }
  __device__ __forceinline__ void side(const SpkArgs& a, int tid, int y, int y_end) {
    ymu[tid] = y < y_end ? a.mu[y] : 0.f;
    yr[tid] = y < y_end ? a.r[y] : 0.f;
  }
  __device__ __forceinline__ void block(int yb, int g) {
    const float4 m = *(const float4*)(ymu + yb * 16 + 4 * g), q = *(const float4*)(yr + yb * 16 + 4 * g);
    ymur[0] = m.x, ymur[1] = m.y, ymur[2] = m.z, ymur[3] = m.w;
    yrr[0] = q.x, yrr[1] = q.y, yrr[2] = q.z, yrr[3] = q.w;
  }
  __device__ __forceinline__ float operator()(float s, int t, int r) const {
    return 0.5f * ((s - xmu[t]) * xr[t] + (s - ymur[r]) * yrr[r]);
  }
};

// (D > 96: 128 and more registers of stationary fragments; two workgroups per CU would spill -- as sv_hist_kernel)
template <int D, class Epi, class Score = LlrScore>
__global__ __launch_bounds__(256, D > 96 ? 1 : 2) void spk_llr_kernel(SpkArgs a) {
  constexpr int YT = kSpkYT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ytile = smem;                        // [YT][D] f32, swizzled
  float* ya = (float*)(smem + YT * D * 4);   // [YT]
  int* yl = (int*)(ya + YT);                 // [YT]
  float* ys = (float*)(yl + YT);             // Score: [YT] per array of its own
  unsigned* h = (unsigned*)((char*)ys + YT * Score::kSide);  // HistEpi: [2][NB]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i = lane & 15;
  // only block pairs with stationary block <= streamed block: a streamed row j counts against i < j
  const int xb0 = blockIdx.y * 256;
  const int y_begin = max((int)blockIdx.x * a.chunk, xb0);
  const int y_end = min(a.S, ((int)blockIdx.x + 1) * a.chunk);
  if (y_begin >= y_end) return;
  const int x0 = xb0 + wave * 64;
  const float c = a.c;

  Epi epi(a, h);
  Score score(a, x0, ys);
  bool nan = false;

  uint4 xf[4][D / 16];
  ap::load_stationary<D>(a.v, a.ld, a.S, x0, xf);
  float xa[4];
  int xl[4];  // (tails on both sides carry label -1)
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int x = x0 + t * 16 + i;
    xa[t] = x < a.S ? a.a[x] : 0.f;
    xl[t] = x < a.S ? a.label[x] : -1;
  }

  ap::stream<D>(
      a.v, a.ld, y_begin, y_end, ytile, xf,
      [&](int y0) {
        if (tid < YT) {
          const int y = y0 + tid;
          ya[tid] = y < y_end ? a.a[y] : 0.f;
          yl[tid] = y < y_end ? a.label[y] : -1;
          score.side(a, tid, y, y_end);
        }
      },
      // a block whose every j <= every i of this wave is skipped; the few blocks that straddle the diagonal are computed whole
      // and lose their tiles below it to the x < y test
      [&](int ybase) { return ybase + 15 > x0; },
      [&](int y0, int yb, const f32x4(&acc)[4]) {
        const float4 yav = *(const float4*)(ya + yb * 16 + 4 * g);
        const int4 ylv = *(const int4*)(yl + yb * 16 + 4 * g);
        const float yar[4] = {yav.x, yav.y, yav.z, yav.w};
        const int ylr[4] = {ylv.x, ylv.y, ylv.z, ylv.w};
        score.block(yb, g);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int x = x0 + t * 16 + i;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int y = y0 + yb * 16 + 4 * g + r;
            if (xl[t] >= 0 && ylr[r] >= 0 && x < y) {
              const float s = score((acc[t][r] + (xa[t] + yar[r])) + c, t, r);
              if (s != s)
                nan = true;
              else
                epi.trial(xl[t] == ylr[r] ? 0 : 1, s);
            }
          }
        }
      });

  epi.finish(a);
  if (nan) atomicOr(a.status, (int32_t)FHVAE_SPK_NAN);
}

template <int D, class Epi, class Score>
int spk_launch(const SpkArgs& a, dim3 grid, hipStream_t st) {
  const int smem = kSpkYT * D * 4 + kSpkYT * (8 + Score::kSide) + (Epi::kHist ? 2 * a.NB * 4 : 0);
  hipError_t e = hipFuncSetAttribute((const void*)spk_llr_kernel<D, Epi, Score>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((spk_llr_kernel<D, Epi, Score>), grid, dim3(256), (size_t)smem, st, a);
  return fh_launch_status();
}

template <class Epi, class Score = LlrScore>
int spk_pairs(SpkArgs a, int64_t D, hipStream_t st) {
  const int64_t nxb = fh_cdiv(a.S, 256);
  a.chunk = (int)fh_allpairs_chunk(a.S, std::max<int64_t>(1, kSpkWorkgroups / nxb), kSpkMinChunk);
  dim3 grid((unsigned)fh_cdiv(a.S, a.chunk), (unsigned)nxb);
  return fh_allpairs_dispatch(D, [&](auto d) { return spk_launch<decltype(d)::value, Epi, Score>(a, grid, st); });
}

__global__ void spk_range_init_kernel(unsigned* keys) {
  if (threadIdx.x < 4) keys[threadIdx.x] = (threadIdx.x & 1) ? 0u : 0xffffffffu;
}
// a key nothing was merged into is no float's: the empty class reads (+inf, -inf)
__global__ void spk_range_done_kernel(const unsigned* __restrict__ keys, float* __restrict__ range) {
  const int t = threadIdx.x;
  if (t >= 4) return;
  const unsigned k = keys[t];
  const bool empty = (t & 1) ? k == 0u : k == 0xffffffffu;
  range[t] = empty ? ((t & 1) ? -INFINITY : INFINITY) : spk_unkey(k);
}

// one thread per row (include/fhvae_spk.h, THE TRANSFORM).  The y_k pass through the row's own part of `out`: a thread reads
// back what it wrote itself.
__global__ __launch_bounds__(64) void spk_project_kernel(const float* __restrict__ x, int64_t ldx, int S, int Din,
                                                         const float* __restrict__ A, int64_t lda, int K,
                                                         const float* __restrict__ mean, int normalise, const float* __restrict__ q,
                                                         const float* __restrict__ scale, float* out, int64_t ldo, float* __restrict__ a) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const float* xr = x + (int64_t)s * ldx;
  float* o = out + (int64_t)s * ldo;
  float nn = 0.f;
  for (int k = 0; k < K; ++k) {
    const float* ar = A + (int64_t)k * lda;
    float acc = 0.f;
    for (int d = 0; d < Din; ++d) {
      const float t = xr[d] - mean[d];
      acc = __builtin_fmaf(ar[d], t, acc);
    }
    nn = __builtin_fmaf(acc, acc, nn);
    o[k] = acc;
  }
  float r = 1.f;
  if (normalise) r = sqrtf((float)K) / fmaxf(sqrtf(nn), 1e-30f);
  float qa = 0.f;
  for (int k = 0; k < K; ++k) {
    float y = o[k];
    if (normalise) y = y * r;
    if (q != nullptr) {
      const float sq = y * y;
      qa = __builtin_fmaf(q[k], sq, qa);
    }
    o[k] = scale != nullptr ? scale[k] * y : y;
  }
  for (int64_t k = K; k < ldo; ++k) o[k] = 0.f;
  if (q != nullptr) a[s] = -qa;
}

// kNorm: the normalised score of include/fhvae_snorm.h from mu, r (S); else the plain one (mu, r unused)
template <bool kNorm>
__global__ void spk_trials_kernel(const float* __restrict__ v, int64_t ld, const float* __restrict__ a, int S, int D, float c,
                                  const int32_t* __restrict__ pairs, int64_t n, float* __restrict__ out, int32_t* status,
                                  const float* __restrict__ mu, const float* __restrict__ r) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int i = pairs[2 * t], j = pairs[2 * t + 1];
  if (i < 0 || i >= S || j < 0 || j >= S) {
    out[t] = NAN;
    atomicOr(status, (int32_t)FHVAE_SPK_BAD_INDEX);
    return;
  }
  const float* vi = v + (int64_t)i * ld;
  const float* vj = v + (int64_t)j * ld;
  float acc = 0.f;
  for (int d = 0; d < D; d += 4) {
    const float4 p = *(const float4*)(vi + d), q = *(const float4*)(vj + d);
    acc = __builtin_fmaf(p.x, q.x, acc);
    acc = __builtin_fmaf(p.y, q.y, acc);
    acc = __builtin_fmaf(p.z, q.z, acc);
    acc = __builtin_fmaf(p.w, q.w, acc);
  }
  const float s = (acc + (a[i] + a[j])) + c;
  out[t] = kNorm ? 0.5f * ((s - mu[i]) * r[i] + (s - mu[j]) * r[j]) : s;
}

// what the three scoring calls check alike
int spk_check(const float* v, int64_t ld, const float* a, int64_t S, int64_t D, const int32_t* status) {
  FH_CHECK_PTR(v);
  FH_CHECK_PTR(a);
  FH_CHECK_PTR(status);
  FH_CHECK_POS(S);
  const int rc = fh_allpairs_check(v, ld, D);
  if (rc != FHVAE_OK) return rc;
  if (((uintptr_t)a & 3) != 0 || ((uintptr_t)status & 3) != 0) return FHVAE_ERR_ALIGN;
  if (S > (int64_t)FHVAE_SPK_MAX_ROWS) return FHVAE_ERR_LIMIT;  // (65536 stationary blocks in the grid's y)
  return FHVAE_OK;
}

}  // namespace

}  // namespace fh

extern "C" int64_t fhvae_spk_ws_bytes(int64_t S, int64_t D) {
  if (S < 1 || S > (int64_t)FHVAE_SPK_MAX_ROWS || D < 16 || D > 128 || D % 16 != 0) return 0;
  return 256;  // the four keys of the range
}

extern "C" int fhvae_spk_project(const float* x, int64_t ldx, int64_t S, int64_t Din, const float* A, int64_t lda, int64_t K,
                                 const float* mean, int normalise, const float* q, const float* scale, float* out, int64_t ldo, float* a,
                                 void* stream) {
  using namespace fh;
  FH_CHECK_PTR(x);
  FH_CHECK_PTR(A);
  FH_CHECK_PTR(mean);
  FH_CHECK_PTR(out);
  if ((q == nullptr) != (a == nullptr)) return FHVAE_ERR_NULL;
  FH_CHECK_POS(S);
  FH_CHECK_POS(Din);
  FH_CHECK_POS(K);
  if (K > 128 || ldx < Din || lda < Din || ldo < K || ldo % 4 != 0) return FHVAE_ERR_SHAPE;
  if ((((uintptr_t)x | (uintptr_t)A | (uintptr_t)mean | (uintptr_t)q | (uintptr_t)scale | (uintptr_t)a) & 3) != 0 || ((uintptr_t)out & 15) != 0)
    return FHVAE_ERR_ALIGN;
  if (Din > FHVAE_SPK_MAX_IN || S > (int64_t)FHVAE_SPK_MAX_ROWS) return FHVAE_ERR_LIMIT;
  hipLaunchKernelGGL(spk_project_kernel, dim3((unsigned)fh_cdiv(S, 64)), dim3(64), 0, (hipStream_t)stream, x, ldx, (int)S, (int)Din, A, lda,
                     (int)K, mean, normalise, q, scale, out, ldo, a);
  return fh_launch_status();
}

namespace fh {

namespace {

// the three scoring calls, shared by the plain score (mu = r = nullptr) and the normalised one
template <class Score>
int spk_range_call(const float* v, int64_t ld, const float* a, const float* mu, const float* r, const int32_t* label, int64_t S, int64_t D,
                   float c, void* ws, int64_t ws_bytes, float* range, int32_t* status, void* stream) {
  FH_CHECK_PTR(label);
  FH_CHECK_PTR(ws);
  FH_CHECK_PTR(range);
  int rc = spk_check(v, ld, a, S, D, status);
  if (rc != FHVAE_OK) return rc;
  if ((((uintptr_t)ws | (uintptr_t)range | (uintptr_t)label) & 3) != 0) return FHVAE_ERR_ALIGN;
  if (ws_bytes < fhvae_spk_ws_bytes(S, D)) return FHVAE_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  SpkArgs g = {};
  g.v = v;
  g.a = a;
  g.label = label;
  g.status = status;
  g.keys = (unsigned*)ws;
  g.ld = ld;
  g.c = c;
  g.S = (int)S;
  g.mu = mu;
  g.r = r;
  hipLaunchKernelGGL(spk_range_init_kernel, dim3(1), dim3(64), 0, st, g.keys);
  rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  if (S > 1) {  // (one row: no trial)
    rc = spk_pairs<RangeEpi, Score>(g, D, st);
    if (rc != FHVAE_OK) return rc;
  }
  hipLaunchKernelGGL(spk_range_done_kernel, dim3(1), dim3(64), 0, st, g.keys, range);
  return fh_launch_status();
}

template <class Score>
int spk_hist_call(const float* v, int64_t ld, const float* a, const float* mu, const float* r, const int32_t* label, int64_t S, int64_t D,
                  float c, float lo, float hi, int64_t n_bins, uint64_t* hist, int32_t* status, void* stream) {
  FH_CHECK_PTR(label);
  FH_CHECK_PTR(hist);
  int rc = spk_check(v, ld, a, S, D, status);
  if (rc != FHVAE_OK) return rc;
  if (n_bins < 64 || n_bins > 8192 || (n_bins & (n_bins - 1)) != 0) return FHVAE_ERR_SHAPE;
  if (!std::isfinite(lo) || !std::isfinite(hi) || hi < lo) return FHVAE_ERR_SHAPE;
  if (((uintptr_t)label & 3) != 0 || ((uintptr_t)hist & 7) != 0) return FHVAE_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  hipError_t he = hipMemsetAsync(hist, 0, (size_t)(2 * n_bins) * sizeof(uint64_t), st);
  if (he != hipSuccess) return (int)he;
  if (S == 1) return FHVAE_OK;  // no trial
  SpkArgs g = {};
  g.v = v;
  g.a = a;
  g.label = label;
  g.status = status;
  g.hist = (unsigned long long*)hist;
  g.ld = ld;
  g.c = c;
  g.lo = lo;
  g.scale = hi == lo ? 0.f : (float)n_bins / (hi - lo);
  g.S = (int)S;
  g.NB = (int)n_bins;
  g.mu = mu;
  g.r = r;
  return spk_pairs<HistEpi, Score>(g, D, st);
}

template <bool kNorm>
int spk_trials_call(const float* v, int64_t ld, const float* a, const float* mu, const float* r, int64_t S, int64_t D, float c,
                    const int32_t* pairs, int64_t n, float* out, int32_t* status, void* stream) {
  FH_CHECK_PTR(pairs);
  FH_CHECK_PTR(out);
  int rc = spk_check(v, ld, a, S, D, status);
  if (rc != FHVAE_OK) return rc;
  FH_CHECK_POS(n);
  if ((((uintptr_t)pairs | (uintptr_t)out) & 3) != 0) return FHVAE_ERR_ALIGN;
  FH_CHECK_I32(n);
  hipLaunchKernelGGL(spk_trials_kernel<kNorm>, dim3((unsigned)fh_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, v, ld, a, (int)S, (int)D, c,
                     pairs, n, out, status, mu, r);
  return fh_launch_status();
}

// mu and r of the normalised calls: given, 4-byte aligned
int sn_check(const float* mu, const float* r) {
  FH_CHECK_PTR(mu);
  FH_CHECK_PTR(r);
  return (((uintptr_t)mu | (uintptr_t)r) & 3) != 0 ? FHVAE_ERR_ALIGN : FHVAE_OK;
}

}  // namespace

}  // namespace fh

extern "C" int fhvae_spk_llr_range(const float* v, int64_t ld, const float* a, const int32_t* label, int64_t S, int64_t D, float c,
                                   void* ws, int64_t ws_bytes, float* range, int32_t* status, void* stream) {
  return fh::spk_range_call<fh::LlrScore>(v, ld, a, nullptr, nullptr, label, S, D, c, ws, ws_bytes, range, status, stream);
}

extern "C" int fhvae_spk_llr_hist(const float* v, int64_t ld, const float* a, const int32_t* label, int64_t S, int64_t D, float c,
                                  float lo, float hi, int64_t n_bins, uint64_t* hist, int32_t* status, void* stream) {
  return fh::spk_hist_call<fh::LlrScore>(v, ld, a, nullptr, nullptr, label, S, D, c, lo, hi, n_bins, hist, status, stream);
}

extern "C" int fhvae_spk_llr_trials(const float* v, int64_t ld, const float* a, int64_t S, int64_t D, float c, const int32_t* pairs,
                                    int64_t n, float* out, int32_t* status, void* stream) {
  return fh::spk_trials_call<false>(v, ld, a, nullptr, nullptr, S, D, c, pairs, n, out, status, stream);
}

// ---- include/fhvae_snorm.h: the same three with the normalised score (its status bits are this file's, value for value)
static_assert((int)FHVAE_SN_NAN == (int)FHVAE_SPK_NAN && (int)FHVAE_SN_BAD_INDEX == (int)FHVAE_SPK_BAD_INDEX &&
                  FHVAE_SN_MAX_ROWS == FHVAE_SPK_MAX_ROWS,
              "fhvae_snorm.h mirrors fhvae_spk.h");

extern "C" int64_t fhvae_sn_ws_bytes(int64_t S, int64_t D) { return fhvae_spk_ws_bytes(S, D); }

extern "C" int fhvae_sn_range(const float* v, int64_t ld, const float* a, const float* mu, const float* r, const int32_t* label, int64_t S,
                              int64_t D, float c, void* ws, int64_t ws_bytes, float* range, int32_t* status, void* stream) {
  const int rc = fh::sn_check(mu, r);
  if (rc != FHVAE_OK) return rc;
  return fh::spk_range_call<fh::NormScore>(v, ld, a, mu, r, label, S, D, c, ws, ws_bytes, range, status, stream);
}

extern "C" int fhvae_sn_hist(const float* v, int64_t ld, const float* a, const float* mu, const float* r, const int32_t* label, int64_t S,
                             int64_t D, float c, float lo, float hi, int64_t n_bins, uint64_t* hist, int32_t* status, void* stream) {
  const int rc = fh::sn_check(mu, r);
  if (rc != FHVAE_OK) return rc;
  return fh::spk_hist_call<fh::NormScore>(v, ld, a, mu, r, label, S, D, c, lo, hi, n_bins, hist, status, stream);
}

extern "C" int fhvae_sn_trials(const float* v, int64_t ld, const float* a, const float* mu, const float* r, int64_t S, int64_t D, float c,
                               const int32_t* pairs, int64_t n, float* out, int32_t* status, void* stream) {
  const int rc = fh::sn_check(mu, r);
  if (rc != FHVAE_OK) return rc;
  return fh::spk_trials_call<true>(v, ld, a, mu, r, S, D, c, pairs, n, out, status, stream);
}
