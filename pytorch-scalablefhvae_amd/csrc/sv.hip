// sv.hip -- speaker verification on embeddings: the histogram of all-pairs cosine scores, split into target and non-target
// trials, in one pass with no (S x S) temporary.
//
//   score(i, j) = (e_i . e_j) / (n_i n_j),  n = max(|e|, 1e-30),  for every i < j with label[i] >= 0 and label[j] >= 0
//   hist[label[i] == label[j] ? 0 : 1][clamp(floor((score + 1) NB / 2), 0, NB - 1)] += 1
//
// The contraction is allpairs_f32.h's pass over the upper triangle, the epilogue a count: every lane turns its four dots of a
// tile into bins and adds 1 to a per-workgroup LDS histogram (ds_add_u32: the LDS serialises lanes that meet in a bin, and
// an integer count has no order); at the end the workgroup adds its non-zero bins to the (2, NB) uint64 result with vector
// 64-bit global atomic adds.  Counts are integers: the result does not depend on the grid or on the order of arrival.
//
// Symmetry, bit for bit: the dot is symmetric (allpairs_f32.h, THE ORDER); the norms come from ONE kernel (sv_norm_kernel, a
// fixed fma chain per row) and enter as the commutative product n_i n_j.  score(i, j) == score(j, i).
#include <algorithm>
#include <cfloat>

#include "allpairs_f32.h"

namespace fh {

namespace {

constexpr int kSvYT = ap::kYT;
constexpr int kSvMinChunk = 512;  // streamed rows per workgroup, at least (a workgroup zeroes and flushes 2 NB bins)
constexpr int kSvWorkgroups = 8192;  // launched workgroups aimed at (about half of them lie below the diagonal and return)

struct SvArgs {
  const float* emb;      // (S, D), leading dimension ld
  const float* nrm;      // (S): max(|e|, 1e-30)
  const int32_t* label;  // (S)
  unsigned long long* hist;  // (2, NB)
  int64_t ld;
  int S, NB, chunk;
};

// n[s] = max(sqrt(sum_d e[s][d]^2), 1e-30): one thread per row, one fma chain in d order
__global__ void sv_norm_kernel(const float* __restrict__ emb, int64_t ld, int S, int D, float* __restrict__ nrm) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const float* p = emb + (int64_t)s * ld;
  float ss = 0.f;
  for (int d = 0; d < D; d += 4) {
    const float4 v = *(const float4*)(p + d);
    ss = __builtin_fmaf(v.x, v.x, ss);
    ss = __builtin_fmaf(v.y, v.y, ss);
    ss = __builtin_fmaf(v.z, v.z, ss);
    ss = __builtin_fmaf(v.w, v.w, ss);
  }
  nrm[s] = fmaxf(sqrtf(ss), 1e-30f);
}

// (D > 96: 128 and more registers of stationary fragments; two workgroups per CU would spill)
template <int D>
__global__ __launch_bounds__(256, D > 96 ? 1 : 2) void sv_hist_kernel(SvArgs a) {
  constexpr int YT = kSvYT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ytile = smem;                               // [YT][D] f32, swizzled
  float* yn = (float*)(smem + YT * D * 4);          // [YT]
  int* yl = (int*)(yn + YT);                        // [YT]
  unsigned* h = (unsigned*)(yl + YT);               // [2][NB]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i = lane & 15;
  // only block pairs with stationary block <= streamed block: a streamed row j counts against i < j
  const int xb0 = blockIdx.y * 256;
  const int y_begin = max((int)blockIdx.x * a.chunk, xb0);
  const int y_end = min(a.S, ((int)blockIdx.x + 1) * a.chunk);
  if (y_begin >= y_end) return;
  const int x0 = xb0 + wave * 64;
  const int NB = a.NB;
  const float half = (float)(NB >> 1), top = (float)(NB - 1);

  for (int e = tid; e < 2 * NB; e += 256) h[e] = 0u;

  uint4 xf[4][D / 16];
  ap::load_stationary<D>(a.emb, a.ld, a.S, x0, xf);
  float xn[4];
  int xl[4];  // (tails on both sides carry label -1)
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int x = x0 + t * 16 + i;
    xn[t] = x < a.S ? a.nrm[x] : 1.f;
    xl[t] = x < a.S ? a.label[x] : -1;
  }

  ap::stream<D>(
      a.emb, a.ld, y_begin, y_end, ytile, xf,
      [&](int y0) {
        if (tid < YT) {
          const int y = y0 + tid;
          yn[tid] = y < y_end ? a.nrm[y] : 1.f;
          yl[tid] = y < y_end ? a.label[y] : -1;
        }
      },
      // a block whose every j <= every i of this wave is skipped; the few blocks that straddle the diagonal are computed whole
      // and lose their tiles below it to the x < y test
      [&](int ybase) { return ybase + 15 > x0; },
      [&](int y0, int yb, const f32x4(&acc)[4]) {
        const float4 ynv = *(const float4*)(yn + yb * 16 + 4 * g);
        const int4 ylv = *(const int4*)(yl + yb * 16 + 4 * g);
        const float ynr[4] = {ynv.x, ynv.y, ynv.z, ynv.w};
        const int ylr[4] = {ylv.x, ylv.y, ylv.z, ylv.w};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int x = x0 + t * 16 + i;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int y = y0 + yb * 16 + 4 * g + r;
            if (xl[t] >= 0 && ylr[r] >= 0 && x < y) {
              // two clamped norms can underflow as a product only when both rows are below 1e-19: the dot is 0 there
              const float score = acc[t][r] / fmaxf(xn[t] * ynr[r], FLT_MIN);
              const float b = fminf(fmaxf(floorf((score + 1.f) * half), 0.f), top);
              atomicAdd(&h[(xl[t] == ylr[r] ? 0 : NB) + (int)b], 1u);
            }
          }
        }
      });

  // ---- flush: a workgroup's count of a bin is below 2^32 (256 * chunk trials); the sum over workgroups is 64-bit
  for (int e = tid; e < 2 * NB; e += 256) {
    const unsigned v = h[e];
    if (v) atomicAdd(a.hist + e, (unsigned long long)v);
  }
}

template <int D>
int sv_launch(const SvArgs& a, dim3 grid, hipStream_t st) {
  const int smem = kSvYT * D * 4 + kSvYT * 8 + 2 * a.NB * 4;
  hipError_t e = hipFuncSetAttribute((const void*)sv_hist_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sv_hist_kernel<D>, grid, dim3(256), (size_t)smem, st, a);
  return fh_launch_status();
}

}  // namespace

}  // namespace fh

extern "C" int64_t fhvae_sv_hist_ws_bytes(int64_t S) {
  if (S < 1) return 0;
  return fh_cdiv(S * (int64_t)sizeof(float), 256) * 256;  // the rows' norms
}

extern "C" int fhvae_sv_hist(const float* emb, int64_t ld, const int32_t* label, int64_t S, int64_t D, int64_t n_bins, void* ws,
                             int64_t ws_bytes, uint64_t* hist, void* stream) {
  using namespace fh;
  FH_CHECK_PTR(emb);
  FH_CHECK_PTR(label);
  FH_CHECK_PTR(hist);
  FH_CHECK_PTR(ws);
  FH_CHECK_POS(S);
  if (n_bins < 64 || n_bins > 8192 || (n_bins & (n_bins - 1)) != 0) return FHVAE_ERR_SHAPE;
  int rc = fh_allpairs_check(emb, ld, D);
  if (rc != FHVAE_OK) return rc;
  if (((uintptr_t)ws & 3) != 0 || ((uintptr_t)hist & 7) != 0) return FHVAE_ERR_ALIGN;
  if (S > ((int64_t)1 << 24)) return FHVAE_ERR_LIMIT;  // (65536 stationary blocks in the grid's y)
  if (ws_bytes < fhvae_sv_hist_ws_bytes(S)) return FHVAE_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  hipError_t he = hipMemsetAsync(hist, 0, (size_t)(2 * n_bins) * sizeof(uint64_t), st);
  if (he != hipSuccess) return (int)he;
  if (S == 1) return FHVAE_OK;  // no trial

  float* nrm = (float*)ws;
  hipLaunchKernelGGL(sv_norm_kernel, dim3((unsigned)fh_cdiv(S, 256)), dim3(256), 0, st, emb, ld, (int)S, (int)D, nrm);
  rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;

  SvArgs a = {};
  a.emb = emb;
  a.nrm = nrm;
  a.label = label;
  a.hist = (unsigned long long*)hist;
  a.ld = ld;
  a.S = (int)S;
  a.NB = (int)n_bins;
  const int64_t nxb = fh_cdiv(S, 256);
  a.chunk = (int)fh_allpairs_chunk(S, std::max<int64_t>(1, kSvWorkgroups / nxb), kSvMinChunk);
  dim3 grid((unsigned)fh_cdiv(S, a.chunk), (unsigned)nxb);
  return fh_allpairs_dispatch(D, [&](auto d) { return sv_launch<decltype(d)::value>(a, grid, st); });
}
