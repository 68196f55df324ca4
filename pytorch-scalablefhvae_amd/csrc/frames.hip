// frames.hip -- the frame-level layer around the inference forward (include/fhvae_frames.h):
//   fhvae_frames_gather       : dense windows (one per `shift` frames, centred, edge-replicated) of a whole corpus cut from the
//                               resident (frames, F) pool, MVN fused, batch-major and / or time-major;
//   fhvae_frames_overlap_mean : per-window values (the decoder's means) back to one row per frame: every frame the mean of the
//                               windows that cover it, the MVN undone.
// Both are streaming kernels: a thread moves V consecutive features of an output row at a time (V = 4: 16-byte accesses, lanes
// along a row and then along the next row, which in the pool, in a window and in `seg` is the next address too, except where
// an utterance or a window ends).  The corpus geometry is two CSR arrays (utt_ptr, win_ptr): a thread finds its utterance by
// binary search (the arrays stay in L2; there is no per-window index tensor to build, upload or keep), re-checks that
// utterance's two CSR entries against each other and against the buffers, and computes every address from them, so no
// argument makes a kernel read or write out of bounds: what does not fit is written as zeros and sets a status bit.
// The overlap mean is a gather (a frame adds its <= ceil(T / shift) windows in increasing window order): no atomics, and
// every element of `seg` is read by exactly one thread.
//
// Arithmetic: f32 with one rounding per operation (no contraction: the pragma below and -ffp-contract=off) and correctly
// rounded division, so the results are bitwise those of the expressions in the header evaluated in numpy float32.
#pragma clang fp contract(off)

#include "common.h"

#include "../../include/fhvae_frames.h"

namespace fh {

constexpr int kFrThreads = 256;

// the last u in [0, U) with ptr[u] <= x (0 when there is none); reads ptr[0 .. U - 1] only
__device__ __forceinline__ int64_t fr_find(const int64_t* __restrict__ ptr, int64_t U, int64_t x) {
  int64_t lo = 0, hi = U - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (ptr[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// utterance u of the two CSR arrays: frames [a, a + n), windows [wa, wa + W); false unless the CSR rule holds
struct FrUtt {
  int64_t a, n, wa, W;
  __device__ __forceinline__ bool load(const int64_t* __restrict__ utt_ptr, const int64_t* __restrict__ win_ptr, int64_t u,
                                       int64_t shift) {
    a = utt_ptr[u];
    wa = win_ptr[u];
    const int64_t e = utt_ptr[u + 1], we = win_ptr[u + 1];
    n = W = 0;
    if (a < 0 || e <= a || wa < 0 || we <= wa) return false;  // (checked before the differences: no entry makes them overflow)
    n = e - a;
    W = we - wa;
    return W == n / shift + (n % shift != 0 ? 1 : 0);
  }
};

// One wave per window: the window index is wave-uniform (readfirstlane), so the search and the CSR checks run once per wave
// on the scalar unit; the wave's lanes then walk the window's T * F / V items, which are consecutive addresses of out_btf
// and, row by row, of the pool and of out_tbf.  (One thread per item, each with its own search and 64-bit index divisions,
// moved 1.7 TB/s at one hour of 80-bin features; see DESIGN.md for what this form moves.)
template <int V>
__global__ void __launch_bounds__(kFrThreads) frames_gather_kernel(const float* __restrict__ pool, int64_t pool_frames,
                                                                   const int64_t* __restrict__ utt_ptr,
                                                                   const int64_t* __restrict__ win_ptr, int64_t U, int64_t w0,
                                                                   int64_t B, int T_, int F, int64_t shift,
                                                                   const float* __restrict__ mean, const float* __restrict__ inv_std,
                                                                   float* __restrict__ out_btf, float* __restrict__ out_tbf,
                                                                   int32_t* status) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * (kFrThreads / 64) + wave;
  if (b >= B) return;
  const int64_t w = w0 + b;
  const int64_t u = fr_find(win_ptr, U, w);
  FrUtt s;
  const bool ok = s.load(utt_ptr, win_ptr, u, shift) && s.n <= pool_frames - s.a && w >= s.wa && w - s.wa < s.W;
  if (!ok && lane == 0) atomicOr(status, FHVAE_FRAMES_BAD_PTR);
  // (k < W = ceil(n / shift): k shift < n + shift, no overflow)
  const int64_t p0 = ok ? (w - s.wa) * shift - T_ / 2 : 0;  // local frame of position 0
  const int FV = F / V, items = T_ * FV;
  // item `it` is features [g V, g V + V) of position t = it / FV: walked without a division per item
  const int dt = 64 / FV, dg = 64 - dt * FV;
  int t = lane / FV, g = lane - t * FV;
  for (int it = lane; it < items; it += 64) {
    const int f = g * V;
    float v[V];
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = 0.f;
    if (ok) {
      int64_t p = p0 + t;
      p = p < 0 ? 0 : (p > s.n - 1 ? s.n - 1 : p);
      const float* src = pool + (s.a + p) * F + f;
      if constexpr (V == 4) {
        const float4 x = *(const float4*)src;
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
      } else {
        v[0] = src[0];
      }
      if (mean) {
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = (v[e] - mean[f + e]) * inv_std[f + e];
      }
    }
    const int64_t o1 = (b * T_ + t) * F + f, o2 = ((int64_t)t * B + b) * F + f;
    if constexpr (V == 4) {
      if (out_btf) *(float4*)(out_btf + o1) = make_float4(v[0], v[1], v[2], v[3]);
      if (out_tbf) *(float4*)(out_tbf + o2) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      if (out_btf) out_btf[o1] = v[0];
      if (out_tbf) out_tbf[o2] = v[0];
    }
    t += dt, g += dg;
    if (g >= FV) g -= FV, ++t;
  }
}

template <int V>
__global__ void __launch_bounds__(kFrThreads) frames_overlap_mean_kernel(const float* __restrict__ seg, int64_t w0, int64_t B,
                                                                         const int64_t* __restrict__ utt_ptr,
                                                                         const int64_t* __restrict__ win_ptr, int64_t U, int64_t g0,
                                                                         int64_t G, int64_t T_, int64_t F, int64_t shift,
                                                                         const float* __restrict__ mean, const float* __restrict__ std,
                                                                         float* __restrict__ out, int32_t* status) {
  const int64_t FV = F / V;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= G * FV) return;
  const int64_t c = (i % FV) * V, r = i / FV;
  const int64_t g = g0 + r;
  const int64_t u = fr_find(utt_ptr, U, g);
  FrUtt s;
  int bad = (s.load(utt_ptr, win_ptr, u, shift) && g >= s.a && g - s.a < s.n) ? 0 : FHVAE_FRAMES_BAD_PTR;
  float v[V];
#pragma unroll
  for (int e = 0; e < V; ++e) v[e] = 0.f;
  if (!bad) {
    const int64_t left = T_ / 2, fl = g - s.a + left;  // (frame f of the utterance is position fl - k shift of window k)
    const int64_t lo = fl - T_ + 1;
    const int64_t k0 = lo <= 0 ? 0 : (lo + shift - 1) / shift;
    const int64_t k1 = fl / shift < s.W - 1 ? fl / shift : s.W - 1;
    if (k1 < k0) {  // (cannot happen for shift <= T - T / 2 and a consistent CSR)
      bad = FHVAE_FRAMES_BAD_PTR;
    } else if (s.wa + k0 < w0 || s.wa + k1 - w0 >= B) {
      bad = FHVAE_FRAMES_BAD_RANGE;
    } else {
      const float* src = seg + ((s.wa + k0 - w0) * T_ + (fl - k0 * shift)) * F + c;
      const int64_t step = (T_ - shift) * F;  // the next window, `shift` positions earlier
      for (int64_t k = k0; k <= k1; ++k, src += step) {
        if constexpr (V == 4) {
          const float4 x = *(const float4*)src;
          if (k == k0) {
            v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
          } else {
            v[0] = v[0] + x.x, v[1] = v[1] + x.y, v[2] = v[2] + x.z, v[3] = v[3] + x.w;
          }
        } else {
          v[0] = k == k0 ? src[0] : v[0] + src[0];
        }
      }
      const float cnt = (float)(k1 - k0 + 1);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        v[e] = v[e] / cnt;
        if (mean) v[e] = v[e] * std[c + e] + mean[c + e];
      }
    }
  }
  if (bad && c == 0) atomicOr(status, bad);
  float* dst = out + r * F + c;
  if constexpr (V == 4) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
  else dst[0] = v[0];
}

// what the two entry points share: the CSR pointers, the status word, the sizes
static inline int frames_common_checks(const int64_t* utt_ptr, const int64_t* win_ptr, int64_t U, int64_t T, int64_t F, int64_t shift,
                                       const float* mean, const float* scale, const int32_t* status) {
  FH_CHECK_PTR(utt_ptr);
  FH_CHECK_PTR(win_ptr);
  FH_CHECK_PTR(status);
  if ((mean == nullptr) != (scale == nullptr)) return FHVAE_ERR_NULL;
  FH_CHECK_POS(U);
  FH_CHECK_POS(T);
  FH_CHECK_POS(F);
  FH_CHECK_POS(shift);
  FH_CHECK_I32(T);
  FH_CHECK_I32(F);
  return FHVAE_OK;
}

}  // namespace fh

using namespace fh;

extern "C" int fhvae_frames_gather(const float* pool, int64_t pool_frames, const int64_t* utt_ptr, const int64_t* win_ptr, int64_t U,
                                   int64_t w0, int64_t B, int64_t T, int64_t F, int64_t shift, const float* mean,
                                   const float* inv_std, float* out_btf, float* out_tbf, int32_t* status, void* stream) {
  FH_CHECK_PTR(pool);
  if (!out_btf && !out_tbf) return FHVAE_ERR_NULL;
  int rc = frames_common_checks(utt_ptr, win_ptr, U, T, F, shift, mean, inv_std, status);
  if (rc != FHVAE_OK) return rc;
  FH_CHECK_POS(pool_frames);
  if (w0 < 0 || B < 0) return FHVAE_ERR_SHAPE;
  if (B == 0) return FHVAE_OK;
  FH_CHECK_I32(B);
  FH_CHECK_I32(T * F);  // (a window's items are counted in int)
  const bool vec = F % 4 == 0 && ((((uintptr_t)pool | (uintptr_t)out_btf | (uintptr_t)out_tbf) & 15) == 0);
  const int64_t blocks = fh_cdiv(B, kFrThreads / 64);  // one wave per window
  hipLaunchKernelGGL(vec ? frames_gather_kernel<4> : frames_gather_kernel<1>, dim3((unsigned)blocks), dim3(kFrThreads), 0,
                     (hipStream_t)stream, pool, pool_frames, utt_ptr, win_ptr, U, w0, B, (int)T, (int)F, shift, mean, inv_std, out_btf,
                     out_tbf, status);
  return fh_launch_status();
}

extern "C" int fhvae_frames_overlap_mean(const float* seg, int64_t w0, int64_t B, const int64_t* utt_ptr, const int64_t* win_ptr,
                                         int64_t U, int64_t g0, int64_t G, int64_t T, int64_t F, int64_t shift, const float* mean,
                                         const float* std, float* out, int32_t* status, void* stream) {
  FH_CHECK_PTR(seg);
  FH_CHECK_PTR(out);
  int rc = frames_common_checks(utt_ptr, win_ptr, U, T, F, shift, mean, std, status);
  if (rc != FHVAE_OK) return rc;
  if (shift > T - T / 2) return FHVAE_ERR_SHAPE;  // a larger shift leaves frames that no window covers
  if (w0 < 0 || g0 < 0 || G < 0) return FHVAE_ERR_SHAPE;
  if (G == 0) return FHVAE_OK;
  FH_CHECK_POS(B);
  FH_CHECK_I32(B);
  const bool vec = F % 4 == 0 && ((((uintptr_t)seg | (uintptr_t)out) & 15) == 0);
  const int64_t blocks = fh_cdiv(G * (vec ? F / 4 : F), kFrThreads);
  FH_CHECK_I32(blocks);
  hipLaunchKernelGGL(vec ? frames_overlap_mean_kernel<4> : frames_overlap_mean_kernel<1>, dim3((unsigned)blocks), dim3(kFrThreads), 0,
                     (hipStream_t)stream, seg, w0, B, utt_ptr, win_ptr, U, g0, G, T, F, shift, mean, std, out, status);
  return fh_launch_status();
}
