// synth.hip -- waveforms from magnitude spectrograms (Griffin-Lim), the way back from csrc/feats.hip's "spec" features.
// librosa 0.8.0 griffinlim / istft semantics for window = periodic Hamming, win_length = n_fft, center = True:
//
//   fhvae_synth_istft    complex spectrum (n_frames, n_bins, 2) -> concatenated waveforms of hop * (frames - 1) samples each.
//                        Launch 1: per frame the windowed inverse DFT as one dense product on the exact-f32 MFMA
//                        (v_mfma_f32_16x16x4_f32): t = spectrum row (1 x K2P, re/im interleaved) . basis^T, basis row n =
//                        window[n] * irfft weights of sample n (host-built, f64 -> f32); the n_fft samples of every frame go
//                        to a workspace.  Launch 2: overlap-add as a gather: every output sample sums the <= ceil(n_fft / hop)
//                        workspace frames that cover it in increasing frame order, divides by the window's sum of squares over
//                        the same frames (where above tiny(f32)); the centre padding is never written.  No atomics.
//   fhvae_synth_project  waveforms -> frames (reflected centre padding, no pre-emphasis) -> forward DFT on the MFMA (the
//                        audio_tile.h product on feats.hip's basis) -> rebuilt = the complex STFT, a = rebuilt - coef * tprev,
//                        next = mag * a / (|a| + 1e-16): one Griffin-Lim round after the inverse, in one launch.
//   fhvae_synth_deemph   x[t] = y[t] + coef x[t-1] per utterance, as a blocked scan: a thread restarts the recurrence from a
//                        zero state W samples before each 256-sample block of the utterance, |coef|^W < 2^-30.
//
// Every output element is a fixed-order f32 chain over values of its own utterance at utterance-relative positions, so the
// result of an utterance does not depend on the rest of the batch or on its place in it: bitwise.
//
// Pointer errors: a check kernel validates wave_ptr / frame_ptr against hop * (frames - 1) and sets FHVAE_SYNTH_BAD_PTR; the
// kernels then write nothing.  They also re-check the utterance of everything they gather, so no input makes them read or
// write out of bounds.
#include "audio_tile.h"

namespace fh {
namespace {

constexpr int kSynThreads = 256;  // 4 waves
constexpr int kSynMaxBM = 64;
using SynTm = TmSet<4, 2, 1>;
constexpr int kDeemphBlock = 256;     // samples per scan block (utterance-relative)
constexpr int kDeemphMaxWarm = 1 << 16;

__global__ void synth_check_kernel(const int64_t* __restrict__ wave_ptr, const int64_t* __restrict__ frame_ptr, int64_t U,
                                   int64_t n_samples, int64_t n_frames, int64_t hop, int32_t* status) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const int64_t w0 = wave_ptr[u], w1 = wave_ptr[u + 1];
  bool ok = w0 >= 0 && w1 <= n_samples && w1 > w0;
  if (frame_ptr) {
    const int64_t f0 = frame_ptr[u], f1 = frame_ptr[u + 1];
    ok = ok && f0 >= 0 && f1 <= n_frames && f1 - f0 >= 2 && w1 - w0 == hop * (f1 - f0 - 1);
    if (u == 0) ok = ok && f0 == 0;
    if (u == U - 1) ok = ok && f1 == n_frames;
  }
  if (u == 0) ok = ok && w0 == 0;
  if (u == U - 1) ok = ok && w1 == n_samples;
  if (!ok) atomicOr(status, FHVAE_SYNTH_BAD_PTR);
}

// ---------------------------------------------------------------------------------------------------- inverse DFT
// LDS: A [BM][LDA], LDA = K2P + 4 (row stride an odd multiple of 16 bytes).  Wave w takes 16-sample groups w, w+4, ... of all
// BM rows (the audio_tile.h scheme).
template <int TM>
__global__ void __launch_bounds__(kSynThreads) synth_idft_kernel(const float* __restrict__ spec, int64_t n_frames,
                                                                const float* __restrict__ basis, int n_fft,
                                                                float* __restrict__ ws, const int32_t* status) {
  constexpr int BM = 16 * TM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if (*status & FHVAE_SYNTH_BAD_PTR) return;
  const int n_bins = n_fft / 2 + 1, K2 = 2 * n_bins, K2P = (K2 + 15) & ~15, LDA = K2P + 4;
  const int KP = (n_fft + 15) & ~15, GN = KP / 16;
  float* A = (float*)smem;
  const int tid = threadIdx.x, lane = tid & 63, wave_id = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int64_t f0 = (int64_t)blockIdx.x * BM;

  for (int e = tid; e < BM * K2P; e += kSynThreads) {
    const int r = e / K2P, k = e - r * K2P;
    float v = 0.f;
    if (f0 + r < n_frames && k < K2) v = spec[(f0 + r) * (int64_t)K2 + k];
    A[r * LDA + k] = v;
  }
  __syncthreads();

  const int NC = K2P / 16;
  for (int g = wave_id; g < GN; g += 4) {
    f32x4 accs[1][TM] = {};
    const float* const br[1] = {basis + (int64_t)(16 * g + i) * K2P + 4 * q};
    tile_product<TM, 1>(accs, br, A + i * LDA + 4 * q, LDA, 0, NC, 1);
    const auto& acc = accs[0];
    // lane (i, q): samples 16g + 4q + v of tile row 16t + i; ws rows are KP wide (the padded samples are written as zeros)
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      const int64_t f = f0 + 16 * t + i;
      if (f < n_frames) *(float4*)(ws + f * KP + 16 * g + 4 * q) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------- overlap-add (gather)
// one thread per output sample
__global__ void __launch_bounds__(256) synth_ola_kernel(const float* __restrict__ ws, const float* __restrict__ win_sq,
                                                        const int64_t* __restrict__ wave_ptr, const int64_t* __restrict__ frame_ptr,
                                                        int64_t U, int64_t n_samples, int64_t n_frames, int n_fft, int hop,
                                                        float* __restrict__ out, const int32_t* status) {
  if (*status & FHVAE_SYNTH_BAD_PTR) return;
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_samples) return;
  const int64_t lo = last_le(wave_ptr, U, s);
  const int64_t w0 = wave_ptr[lo], w1 = wave_ptr[lo + 1], p0 = frame_ptr[lo], p1 = frame_ptr[lo + 1];
  const int64_t F = p1 - p0;
  if (!(w0 <= s && s < w1 && w1 <= n_samples && p0 >= 0 && p1 <= n_frames && F >= 2 && w1 - w0 == (int64_t)hop * (F - 1))) return;
  const int KP = (n_fft + 15) & ~15;
  const int64_t p = s - w0 + n_fft / 2;  // position in the padded signal
  int64_t fa = p - n_fft + 1;
  fa = fa <= 0 ? 0 : (fa + hop - 1) / hop;  // first frame with fa * hop + n_fft > p
  int64_t fb = p / hop;                     // last frame with fb * hop <= p
  fb = fb > F - 1 ? F - 1 : fb;
  float acc = 0.f, wss = 0.f;
  for (int64_t f = fa; f <= fb; ++f) {
    const int j = (int)(p - f * hop);
    acc += ws[(p0 + f) * KP + j];
    wss += win_sq[j];
  }
  out[s] = wss > 1.17549435e-38f ? acc / wss : acc;  // librosa.istft: divide where the envelope exceeds tiny(float32)
}

// ---------------------------------------------------------------------------------------------------- project
// The feats.hip spec tile without the pre-emphasis, with the complex result kept.  Reflection is numpy's "reflect" for any
// pad length (period 2 (L - 1)); frame f of an utterance of F frames reads padded positions f * hop .. f * hop + n_fft - 1,
// which for odd n_fft reaches one sample past the symmetric padding.
template <int TM>
__global__ void __launch_bounds__(kSynThreads) synth_project_kernel(const float* __restrict__ wave, const int64_t* __restrict__ wave_ptr,
                                                                   const int64_t* __restrict__ frame_ptr, int64_t U, int64_t n_samples,
                                                                   int64_t n_frames, const float* __restrict__ dft,
                                                                   const float* __restrict__ mag, const float* __restrict__ tprev,
                                                                   float coef, int n_fft, int hop, float* __restrict__ rebuilt,
                                                                   float* __restrict__ next, const int32_t* status) {
  constexpr int BM = 16 * TM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int64_t row_base[BM], row_start[BM], row_len[BM];
  __shared__ int row_ok[BM];
  if (*status & FHVAE_SYNTH_BAD_PTR) return;
  const int KP = (n_fft + 15) & ~15, LDA = KP + 4;
  const int n_bins = n_fft / 2 + 1, G = (n_bins + 15) / 16;
  const int pad = n_fft / 2;
  float* A = (float*)smem;
  const int tid = threadIdx.x, lane = tid & 63, wave_id = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int64_t f0 = (int64_t)blockIdx.x * BM;

  if (tid < BM) {
    const int64_t f = f0 + tid;
    int ok = 0;
    int64_t base = 0, start = 0, L = 0;
    if (f < n_frames) {
      const int64_t lo = last_le(frame_ptr, U, f);
      const int64_t w0 = wave_ptr[lo], w1 = wave_ptr[lo + 1], p0 = frame_ptr[lo], p1 = frame_ptr[lo + 1];
      L = w1 - w0;
      ok = w0 >= 0 && w1 <= n_samples && L >= 1 && p0 <= f && f < p1 && p1 - p0 >= 2 && L == (int64_t)hop * (p1 - p0 - 1);
      base = w0;
      start = (f - p0) * hop - pad;
    }
    row_ok[tid] = ok;
    row_base[tid] = base;
    row_start[tid] = start;
    row_len[tid] = L;
  }
  __syncthreads();

  for (int e = tid; e < BM * KP; e += kSynThreads) {
    const int r = e / KP, k = e - r * KP;
    float v = 0.f;
    if (row_ok[r] && k < n_fft) {
      const int64_t L = row_len[r];
      int64_t p = row_start[r] + k;
      if (p < 0 || p >= L) {
        const int64_t period = 2 * (L - 1);
        if (period == 0) {
          p = 0;
        } else {
          p %= period;
          p = p < 0 ? p + period : p;
          p = p >= L ? period - p : p;
        }
      }
      v = wave[row_base[r] + p];
    }
    A[r * LDA + k] = v;
  }
  __syncthreads();

  const int NC = KP / 16;
  for (int g = wave_id; g < G; g += 4) {
    f32x4 acc[2][TM] = {};
    const float* bc = dft + (int64_t)(32 * g + i) * KP + 4 * q;
    const float* const bcs[2] = {bc, bc + (int64_t)16 * KP};
    tile_product<TM, 2>(acc, bcs, A + i * LDA + 4 * q, LDA, 0, NC, 1);
    const auto &ac = acc[0], &as = acc[1];
    // lane (i, q): bins 16g + 4q + v of tile row 16t + i
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      const int r = 16 * t + i;
      if (!row_ok[r]) continue;
      const int64_t row = (f0 + r) * (int64_t)n_bins;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int bin = 16 * g + 4 * q + v;
        if (bin >= n_bins) continue;
        const float re = ac[t][v], im = as[t][v];
        float are = re, aim = im;
        if (tprev) {
          const float2 tp = *(const float2*)(tprev + 2 * (row + bin));
          are = __builtin_fmaf(-coef, tp.x, re);
          aim = __builtin_fmaf(-coef, tp.y, im);
        }
        if (rebuilt) *(float2*)(rebuilt + 2 * (row + bin)) = make_float2(re, im);
        const float sc = mag[row + bin] / (__builtin_sqrtf(__builtin_fmaf(are, are, aim * aim)) + 1e-16f);
        *(float2*)(next + 2 * (row + bin)) = make_float2(are * sc, aim * sc);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- de-emphasis
// one thread per kDeemphBlock consecutive samples of the concatenation; the recurrence restarts (zero state, `warm` samples
// earlier, never before the utterance's start) at every multiple of kDeemphBlock of the utterance-relative position, so a
// sample's chain depends on its utterance alone.
__global__ void __launch_bounds__(256) synth_deemph_kernel(const float* __restrict__ y, const int64_t* __restrict__ wave_ptr,
                                                           int64_t U, int64_t n_samples, float coef, int warm,
                                                           float* __restrict__ out, const int32_t* status) {
  if (*status & FHVAE_SYNTH_BAD_PTR) return;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t t = g * kDeemphBlock;
  if (t >= n_samples) return;
  const int64_t end = t + kDeemphBlock < n_samples ? t + kDeemphBlock : n_samples;
  int64_t u = last_le(wave_ptr, U, t);
  while (t < end && u < U) {
    const int64_t w0 = wave_ptr[u], w1 = wave_ptr[u + 1];
    if (w0 < 0 || w1 > n_samples || w0 > t) return;  // (the check kernel has flagged it)
    if (t >= w1) {
      ++u;
      continue;
    }
    const int64_t r = t - w0, b = r - r % kDeemphBlock;
    const int64_t s = b > warm ? b - warm : 0;
    int64_t stop = w0 + b + kDeemphBlock;
    stop = stop > w1 ? w1 : stop;
    stop = stop > end ? end : stop;
    float x = 0.f;
    for (int64_t k = w0 + s; k < t; ++k) x = __builtin_fmaf(coef, x, y[k]);
    for (int64_t k = t; k < stop; ++k) {
      x = __builtin_fmaf(coef, x, y[k]);
      out[k] = x;
    }
    t = stop;
  }
}

static inline int64_t synth_smem(int BM, int64_t cols) { return (int64_t)BM * 4 * (cols + 4); }
constexpr int64_t kSynStaticLds = kSynMaxBM * (3 * 8 + 4);

// the widest tile both products of a round fit in LDS with (K2P >= KP: the inverse's rows are the longer ones)
static inline int synth_tm(int64_t n_fft) {
  const int64_t K2P = (2 * (n_fft / 2 + 1) + 15) & ~15LL;
  return SynTm::largest(kCuLdsBytes, [&](int BM) { return synth_smem(BM, K2P) + kSynStaticLds; });
}

// the size checks every entry point shares; FHVAE_OK or the error to return before any launch
static int synth_sizes_ok(int64_t n_fft, int64_t hop, int64_t U, int64_t n_samples, int64_t n_frames) {
  FH_CHECK_POS(n_samples);
  FH_CHECK_POS(U);
  FH_CHECK_POS(n_frames);
  FH_CHECK_POS(hop);
  if (n_fft < 2 || n_fft > FHVAE_FEATS_MAX_NFFT || hop > n_fft) return FHVAE_ERR_LIMIT;
  if (synth_tm(n_fft) == 0) return FHVAE_ERR_LIMIT;
  FH_CHECK_I32(fh_cdiv(n_frames, 16));
  FH_CHECK_I32(fh_cdiv(n_samples, 256));
  FH_CHECK_I32(fh_cdiv(U, 256));
  return FHVAE_OK;
}

}  // namespace
}  // namespace fh

using namespace fh;

extern "C" int fhvae_synth_tile_rows(int64_t n_fft) {
  if (n_fft < 2 || n_fft > FHVAE_FEATS_MAX_NFFT) return 0;
  return 16 * synth_tm(n_fft);
}

extern "C" int fhvae_synth_istft(const float* spec, int64_t n_frames, const int64_t* wave_ptr, const int64_t* frame_ptr, int64_t U,
                                 int64_t n_samples, const float* synth_basis, const float* win_sq, int64_t n_fft, int64_t hop,
                                 float* frames_ws, float* wave_out, int32_t* status, void* stream) {
  FH_CHECK_PTR(spec);
  FH_CHECK_PTR(wave_ptr);
  FH_CHECK_PTR(frame_ptr);
  FH_CHECK_PTR(synth_basis);
  FH_CHECK_PTR(win_sq);
  FH_CHECK_PTR(frames_ws);
  FH_CHECK_PTR(wave_out);
  FH_CHECK_PTR(status);
  int rc = synth_sizes_ok(n_fft, hop, U, n_samples, n_frames);
  if (rc != FHVAE_OK) return rc;
  if ((((uintptr_t)synth_basis) & 15) != 0 || (((uintptr_t)frames_ws) & 15) != 0) return FHVAE_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(synth_check_kernel, dim3((unsigned)fh_cdiv(U, 256)), dim3(256), 0, s, wave_ptr, frame_ptr, U, n_samples,
                     n_frames, hop, status);
  rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  const int nf = (int)n_fft;
  rc = SynTm::dispatch(synth_tm(n_fft), [&](auto tmc) {
    constexpr int TM = decltype(tmc)::value;
    return launch_lds(synth_idft_kernel<TM>, fh_cdiv(n_frames, 16 * TM), kSynThreads, synth_smem(16 * TM, (2 * (nf / 2 + 1) + 15) & ~15),
                      s, spec, n_frames, synth_basis, nf, frames_ws, status);
  });
  if (rc != FHVAE_OK) return rc;
  hipLaunchKernelGGL(synth_ola_kernel, dim3((unsigned)fh_cdiv(n_samples, 256)), dim3(256), 0, s, frames_ws, win_sq, wave_ptr,
                     frame_ptr, U, n_samples, n_frames, nf, (int)hop, wave_out, status);
  return fh_launch_status();
}

extern "C" int fhvae_synth_project(const float* wave, int64_t n_samples, const int64_t* wave_ptr, const int64_t* frame_ptr, int64_t U,
                                   int64_t n_frames, const float* dft_basis, const float* mag, const float* tprev, float coef,
                                   int64_t n_fft, int64_t hop, float* rebuilt, float* next, int32_t* status, void* stream) {
  FH_CHECK_PTR(wave);
  FH_CHECK_PTR(wave_ptr);
  FH_CHECK_PTR(frame_ptr);
  FH_CHECK_PTR(dft_basis);
  FH_CHECK_PTR(mag);
  FH_CHECK_PTR(next);
  FH_CHECK_PTR(status);
  int rc = synth_sizes_ok(n_fft, hop, U, n_samples, n_frames);
  if (rc != FHVAE_OK) return rc;
  if ((((uintptr_t)dft_basis) & 15) != 0) return FHVAE_ERR_ALIGN;
  if ((((uintptr_t)next) & 7) != 0 || (((uintptr_t)tprev) & 7) != 0 || (((uintptr_t)rebuilt) & 7) != 0) return FHVAE_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(synth_check_kernel, dim3((unsigned)fh_cdiv(U, 256)), dim3(256), 0, s, wave_ptr, frame_ptr, U, n_samples,
                     n_frames, hop, status);
  rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  const int nf = (int)n_fft;
  return SynTm::dispatch(synth_tm(n_fft), [&](auto tmc) {
    constexpr int TM = decltype(tmc)::value;
    return launch_lds(synth_project_kernel<TM>, fh_cdiv(n_frames, 16 * TM), kSynThreads, synth_smem(16 * TM, (nf + 15) & ~15), s, wave,
                      wave_ptr, frame_ptr, U, n_samples, n_frames, dft_basis, mag, tprev, coef, nf, (int)hop, rebuilt, next, status);
  });
}

extern "C" int fhvae_synth_deemph(const float* wave, const int64_t* wave_ptr, int64_t U, int64_t n_samples, float coef, float* out,
                                  int32_t* status, void* stream) {
  FH_CHECK_PTR(wave);
  FH_CHECK_PTR(wave_ptr);
  FH_CHECK_PTR(out);
  FH_CHECK_PTR(status);
  FH_CHECK_POS(n_samples);
  FH_CHECK_POS(U);
  const float a = coef < 0.f ? -coef : coef;
  if (!(a < 1.f)) return FHVAE_ERR_LIMIT;  // (NaN too)
  // |coef|^warm < 2^-30: what the restart drops is below f32 resolution of the running value
  int64_t warm = 0;
  if (a > 0.f) {
    const double w = __builtin_ceil(-30.0 * 0.6931471805599453 / __builtin_log((double)a));
    if (w > (double)kDeemphMaxWarm) return FHVAE_ERR_LIMIT;
    warm = (int64_t)w;
  }
  FH_CHECK_I32(fh_cdiv(fh_cdiv(n_samples, kDeemphBlock), 256));
  FH_CHECK_I32(fh_cdiv(U, 256));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(synth_check_kernel, dim3((unsigned)fh_cdiv(U, 256)), dim3(256), 0, s, wave_ptr, (const int64_t*)nullptr, U,
                     n_samples, (int64_t)0, (int64_t)1, status);
  int rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  hipLaunchKernelGGL(synth_deemph_kernel, dim3((unsigned)fh_cdiv(fh_cdiv(n_samples, kDeemphBlock), 256)), dim3(256), 0, s, wave,
                     wave_ptr, U, n_samples, coef, (int)warm, out, status);
  return fh_launch_status();
}
