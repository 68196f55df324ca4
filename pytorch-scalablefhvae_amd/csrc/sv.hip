// sv.hip -- speaker verification on embeddings: the histogram of all-pairs cosine scores, split into target and non-target
// trials, in one pass with no (S x S) temporary.
//
//   score(i, j) = (e_i . e_j) / (n_i n_j),  n = max(|e|, 1e-30),  for every i < j with label[i] >= 0 and label[j] >= 0
//   hist[label[i] == label[j] ? 0 : 1][clamp(floor((score + 1) NB / 2), 0, NB - 1)] += 1
//
// The contraction is disc_mfma.hip's MODE 0: a workgroup keeps 256 STATIONARY rows (64 per wave, as MFMA B-operand fragments
// in registers) and streams a chunk of the same matrix through LDS in tiles of 64 (same swizzle), exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32), epilogue on the VALU.  The epilogue here is a count: every lane turns its four dots into bins and
// adds 1 to a per-workgroup LDS histogram (ds_add_u32: the LDS serialises lanes that meet in a bin, and an integer count
// has no order); at the end the workgroup adds its non-zero bins to the (2, NB) uint64 result with vector 64-bit global
// atomic adds.  Counts are integers: the result does not depend on the grid or on the order of arrival.
//
// Symmetry, bit for bit: the k order of the MFMA chain is the same whichever row is stationary (both operands use the
// lane (g, i) <-> d = 16 jj + 4 g + c layout) and a product of two floats commutes; the norms come from ONE kernel
// (sv_norm_kernel, a fixed fma chain per row) and enter as the commutative product n_i n_j.  score(i, j) == score(j, i).
#include <algorithm>
#include <cfloat>

#include "common.h"

namespace fh {

namespace {

constexpr int kSvYT = 64;         // streamed rows per LDS tile
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

template <int D>
__device__ __forceinline__ int sv_yoff(int row, int ch) {  // byte offset of 16-byte chunk ch of LDS row `row` (disc_mfma.hip's swizzle)
  constexpr int CHN = D / 4;
  return row * (D * 4) + ((ch ^ (row & (CHN % 8 == 0 ? 7 : 3))) << 4);  // (stays inside an aligned group of 8 / 4 chunks: any D % 16 == 0)
}

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
  constexpr int CHN = D / 4;  // 16-byte chunks per row
  constexpr int NJ = D / 16;  // 16-k groups
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

  // ---- stationary fragments: lane (g,i) of tile t holds X[x0+16t+i][4g+16jj .. +3]; rows past S carry label -1
  uint4 xf[4][NJ];
  float xn[4];
  int xl[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int x = x0 + t * 16 + i;
    const bool ok = x < a.S;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
      uint4 u = make_uint4(0, 0, 0, 0);
      if (ok) u = *(const uint4*)(a.emb + (int64_t)x * a.ld + 4 * g + 16 * jj);
      xf[t][jj] = u;
    }
    xn[t] = ok ? a.nrm[x] : 1.f;
    xl[t] = ok ? a.label[x] : -1;
  }

  // ---- stream the chunk in tiles of 64 rows
  constexpr int LOADS = YT * CHN / 256;  // 16-byte chunks per thread per tile
  uint4 st[LOADS];
  auto issue = [&](int y0) {
#pragma unroll
    for (int p = 0; p < LOADS; ++p) {
      const int id = tid + p * 256;
      const int row = id / CHN, ch = id % CHN;
      const int y = y0 + row;
      st[p] = (y < y_end) ? *(const uint4*)(a.emb + (int64_t)y * a.ld + ch * 4) : make_uint4(0, 0, 0, 0);
    }
  };
  issue(y_begin);
  for (int y0 = y_begin; y0 < y_end; y0 += YT) {
#pragma unroll
    for (int p = 0; p < LOADS; ++p) {
      const int id = tid + p * 256;
      *(uint4*)(ytile + sv_yoff<D>(id / CHN, id % CHN)) = st[p];
    }
    if (tid < YT) {
      const int y = y0 + tid;
      const bool ok = y < y_end;
      yn[tid] = ok ? a.nrm[y] : 1.f;
      yl[tid] = ok ? a.label[y] : -1;
    }
    __syncthreads();
    if (y0 + YT < y_end) issue(y0 + YT);

#pragma unroll 1
    for (int yb = 0; yb < YT / 16; ++yb) {
      const int ybase = y0 + yb * 16;
      if (ybase >= y_end) break;
      if (ybase + 15 <= x0) continue;  // every j of this block <= every i of this wave
      // A fragments: Y[yb*16+i][4g+16jj .. +3]
      uint4 af[NJ];
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) af[jj] = *(const uint4*)(ytile + sv_yoff<D>(yb * 16 + i, g + 4 * jj));
      const float4 ynv = *(const float4*)(yn + yb * 16 + 4 * g);
      const int4 ylv = *(const int4*)(yl + yb * 16 + 4 * g);
      const float ynr[4] = {ynv.x, ynv.y, ynv.z, ynv.w};
      const int ylr[4] = {ylv.x, ylv.y, ylv.z, ylv.w};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (ybase + 15 <= x0 + 16 * t) continue;  // (uniform over the wave)
        // dot tile: col = lane & 15 -> stationary row x0+16t+i, accumulator r -> streamed row ybase+4g+r
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
          const uint4 ua = af[jj], ub = xf[t][jj];
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ua.x), __uint_as_float(ub.x), acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ua.y), __uint_as_float(ub.y), acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ua.z), __uint_as_float(ub.z), acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ua.w), __uint_as_float(ub.w), acc, 0, 0, 0);
        }
        const int x = x0 + t * 16 + i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int y = ybase + 4 * g + r;
          if (xl[t] >= 0 && ylr[r] >= 0 && x < y) {  // (tails on both sides carry label -1)
            // two clamped norms can underflow as a product only when both rows are below 1e-19: the dot is 0 there
            const float score = acc[r] / fmaxf(xn[t] * ynr[r], FLT_MIN);
            const float b = fminf(fmaxf(floorf((score + 1.f) * half), 0.f), top);
            atomicAdd(&h[(xl[t] == ylr[r] ? 0 : NB) + (int)b], 1u);
          }
        }
      }
    }
    __syncthreads();
  }

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
  if (D < 16 || D > 128 || D % 16 != 0) return FHVAE_ERR_SHAPE;
  if (n_bins < 64 || n_bins > 8192 || (n_bins & (n_bins - 1)) != 0) return FHVAE_ERR_SHAPE;
  if (ld < D) return FHVAE_ERR_SHAPE;
  if (ld % 4 != 0 || ((uintptr_t)emb & 15) != 0 || ((uintptr_t)ws & 3) != 0 || ((uintptr_t)hist & 7) != 0) return FHVAE_ERR_ALIGN;
  if (S > ((int64_t)1 << 24)) return FHVAE_ERR_LIMIT;  // (65536 stationary blocks in the grid's y)
  if (ws_bytes < fhvae_sv_hist_ws_bytes(S)) return FHVAE_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  hipError_t he = hipMemsetAsync(hist, 0, (size_t)(2 * n_bins) * sizeof(uint64_t), st);
  if (he != hipSuccess) return (int)he;
  if (S == 1) return FHVAE_OK;  // no trial

  float* nrm = (float*)ws;
  hipLaunchKernelGGL(sv_norm_kernel, dim3((unsigned)fh_cdiv(S, 256)), dim3(256), 0, st, emb, ld, (int)S, (int)D, nrm);
  int rc = fh_launch_status();
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
  const int64_t want = std::max<int64_t>(1, kSvWorkgroups / nxb);
  a.chunk = (int)std::max<int64_t>(kSvMinChunk, fh_cdiv(fh_cdiv(S, want), kSvYT) * kSvYT);
  dim3 grid((unsigned)fh_cdiv(S, a.chunk), (unsigned)nxb);
  switch (D) {
    case 16: return sv_launch<16>(a, grid, st);
    case 32: return sv_launch<32>(a, grid, st);
    case 48: return sv_launch<48>(a, grid, st);
    case 64: return sv_launch<64>(a, grid, st);
    case 80: return sv_launch<80>(a, grid, st);
    case 96: return sv_launch<96>(a, grid, st);
    case 112: return sv_launch<112>(a, grid, st);
    default: return sv_launch<128>(a, grid, st);
  }
}
