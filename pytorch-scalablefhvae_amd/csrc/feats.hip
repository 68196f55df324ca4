// feats.hip -- log-mel (fbank) and log-magnitude (spec) features of a batch of utterances in one launch
// (the GPU form of the reference's prepare_numpy_data.generate_feat on AudioUtils.rstft / to_melspec, utils.py:155-272).
//
// Per frame the work is two dense products on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32):
//   DFT:  [c | s] = frame (1 x KP) . basis^T      the basis rows are the windowed cos / -sin columns (host-built, f64 -> f32)
//   mel:  M = |c + i s| (1 x NBP) . mel^T         fbank only
// then log and the floor.  A workgroup takes BM = 16*TM consecutive output rows (frames); a tile may span utterances, each
// row finds its utterance by binary search in frame_ptr.  Pre-emphasis and the reflection of the centre padding are applied
// while the tile is gathered into LDS (one row per frame, KP = n_fft rounded up to 16, zero-filled).  Each wave owns whole
// 16-bin groups (16 cos + 16 sin basis rows) for all BM rows and multiplies them by the shared row-tile product
// (audio_tile.h: tile_product).  The magnitudes go to LDS for the mel product (same product, 16-mel groups).
//
// Every output element is a fixed-order f32 chain over its own row's samples (chunk, then k-step, then lane group: the MFMA
// order), so a frame's result does not depend on the other frames of its launch or its place in the tile: bitwise.
//
// Pointer errors: a check kernel validates wave_ptr / frame_ptr against the framing rule and sets FHVAE_FEATS_BAD_PTR; the
// main kernel then writes nothing.  It also re-checks the utterance of every row it gathers, so no input makes it read or
// write out of bounds.
#include "audio_tile.h"

namespace fh {

constexpr int kFeatThreads = 256;  // 4 waves
constexpr int kFeatMaxBM = 64;
using FeatTm = TmSet<4, 2, 1>;

__host__ __device__ inline int64_t feats_frames(int64_t L, int64_t n_fft, int64_t hop) {
  const int64_t pad = n_fft / 2;
  return 1 + (L + 2 * pad - n_fft) / hop;  // prepare step 3; L >= pad + 1 keeps the numerator >= 0
}

// one thread per utterance: monotone pointers, enough samples for one reflection, frame counts by the framing rule
__global__ void feats_check_kernel(const int64_t* __restrict__ wave_ptr, const int64_t* __restrict__ frame_ptr, int64_t U,
                                   int64_t n_samples, int64_t n_frames, int64_t n_fft, int64_t hop, int32_t* status) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const int64_t w0 = wave_ptr[u], w1 = wave_ptr[u + 1], f0 = frame_ptr[u], f1 = frame_ptr[u + 1];
  bool ok = w0 >= 0 && w1 <= n_samples && w1 - w0 >= n_fft / 2 + 1;
  ok = ok && f0 >= 0 && f1 <= n_frames && f1 - f0 == (ok ? feats_frames(w1 - w0, n_fft, hop) : -1);
  if (u == 0) ok = ok && f0 == 0;
  if (u == U - 1) ok = ok && f1 == n_frames;
  if (!ok) atomicOr(status, FHVAE_FEATS_BAD_PTR);
}

// FBANK: 1 = log-mel, 0 = log-magnitude spectrogram.  LDS: frames [BM][LDA] (LDA = KP + 4: row stride an odd multiple of
// 16 bytes, so the 16 rows of a ds_read_b128 fragment hit 16 distinct bank slots), then for fbank mags [BM][LDM].
template <int TM, bool FBANK>
__global__ void __launch_bounds__(kFeatThreads) feats_kernel(const float* __restrict__ wave, const int64_t* __restrict__ wave_ptr,
                                                             const int64_t* __restrict__ frame_ptr, int64_t U, int64_t n_samples,
                                                             int64_t n_frames, const float* __restrict__ dft,
                                                             const float* __restrict__ melb, int n_fft, int hop, int n_out,
                                                             float* __restrict__ out, const int32_t* status) {
  constexpr int BM = 16 * TM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int64_t row_base[BM], row_start[BM], row_len[BM];
  __shared__ int row_ok[BM];
  if (*status & FHVAE_FEATS_BAD_PTR) return;  // (set by the check kernel: the rows would not be unique)
  const int KP = (n_fft + 15) & ~15, LDA = KP + 4;
  const int n_bins = n_fft / 2 + 1, G = (n_bins + 15) / 16, NBP = 16 * G, LDM = NBP + 4;
  const int pad = n_fft / 2;
  float* A = (float*)smem;
  float* Ms = A + BM * LDA;
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
      ok = w0 >= 0 && w1 <= n_samples && L >= pad + 1 && p0 <= f && f < p1 && p1 - p0 == feats_frames(L, n_fft, hop);
      base = w0;
      start = (f - p0) * hop - pad;  // first sample of the frame in unpadded coordinates
    }
    row_ok[tid] = ok;
    row_base[tid] = base;
    row_start[tid] = start;
    row_len[tid] = L;
  }
  __syncthreads();

  // gather: A[r][k] = y'(start_r + k) with y'[t] = y[t] - 0.97 y[t-1] (y[-1] = 0) and reflect padding; 0 for k >= n_fft
  for (int e = tid; e < BM * KP; e += kFeatThreads) {
    const int r = e / KP, k = e - r * KP;
    float v = 0.f;
    if (row_ok[r] && k < n_fft) {
      const int64_t L = row_len[r];
      int64_t p = row_start[r] + k;
      p = p < 0 ? -p : p;
      p = p >= L ? 2 * L - 2 - p : p;  // one reflection suffices for L >= pad + 1
      const float* y = wave + row_base[r];
      const float prev = p > 0 ? y[p - 1] : 0.f;
      v = __builtin_fmaf(-0.97f, prev, y[p]);
    }
    A[r * LDA + k] = v;
  }
  __syncthreads();

  const int NC = KP / 16;
  // ---- DFT: wave w takes bin groups w, w+4, ...
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
      float m[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) m[v] = __builtin_sqrtf(__builtin_fmaf(ac[t][v], ac[t][v], as[t][v] * as[t][v]));
      if constexpr (FBANK) {
        *(float4*)(Ms + r * LDM + 16 * g + 4 * q) = make_float4(m[0], m[1], m[2], m[3]);  // padded bins: zero basis rows -> 0
      } else {
        if (row_ok[r]) {
          float* o = out + (f0 + r) * (int64_t)n_out;
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int bin = 16 * g + 4 * q + v;
            if (bin < n_bins) o[bin] = fmaxf(logf(m[v]), -50.f);  // utils.py:219-221
          }
        }
      }
    }
  }
  if constexpr (FBANK) {
    __syncthreads();
    // ---- mel: M[r][j] = sum over bins of mag[r][bin] * mel[j][bin]; wave w takes mel groups w, w+4, ...
    const int H = (n_out + 15) / 16, NCM = NBP / 16;
    for (int h = wave_id; h < H; h += 4) {
      f32x4 accm[1][TM] = {};
      const float* const br[1] = {melb + (int64_t)(16 * h + i) * NBP + 4 * q};
      tile_product<TM, 1>(accm, br, Ms + i * LDM + 4 * q, LDM, 0, NCM, 1);
      const auto& acc = accm[0];
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        const int r = 16 * t + i;
        if (!row_ok[r]) continue;
        float* o = out + (f0 + r) * (int64_t)n_out;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int j = 16 * h + 4 * q + v;
          if (j < n_out) o[j] = fmaxf(logf(acc[t][v]), -20.f);  // utils.py:266-270
        }
      }
    }
  }
}

// LDS bytes of the dynamic part for a BM-row tile
static inline int64_t feats_smem(int BM, int64_t n_fft, bool fbank) {
  const int64_t KP = (n_fft + 15) & ~15LL, NBP = 16 * ((n_fft / 2 + 1 + 15) / 16);
  return (int64_t)BM * 4 * ((KP + 4) + (fbank ? NBP + 4 : 0));
}
constexpr int64_t kFeatStaticLds = kFeatMaxBM * (3 * 8 + 4);

static inline int feats_tm(int64_t n_fft, bool fbank) {
  return FeatTm::largest(kCuLdsBytes, [&](int BM) { return feats_smem(BM, n_fft, fbank) + kFeatStaticLds; });
}

}  // namespace fh

using namespace fh;

extern "C" int fhvae_feats_tile_rows(int64_t n_fft, int ftype) {
  if (n_fft < 2 || n_fft > FHVAE_FEATS_MAX_NFFT || (ftype != FHVAE_FEATS_FBANK && ftype != FHVAE_FEATS_SPEC)) return 0;
  return 16 * feats_tm(n_fft, ftype == FHVAE_FEATS_FBANK);
}

extern "C" int fhvae_feats_fwd(const float* wave, int64_t n_samples, const int64_t* wave_ptr, const int64_t* frame_ptr, int64_t U,
                               int64_t n_frames, const float* dft_basis, const float* mel_basis, int64_t n_fft, int64_t hop,
                               int64_t n_mels, int ftype, float* out, int32_t* status, void* stream) {
  FH_CHECK_PTR(wave);
  FH_CHECK_PTR(wave_ptr);
  FH_CHECK_PTR(frame_ptr);
  FH_CHECK_PTR(dft_basis);
  FH_CHECK_PTR(out);
  FH_CHECK_PTR(status);
  if (ftype != FHVAE_FEATS_FBANK && ftype != FHVAE_FEATS_SPEC) return FHVAE_ERR_DTYPE;
  const bool fbank = ftype == FHVAE_FEATS_FBANK;
  if (fbank) FH_CHECK_PTR(mel_basis);
  FH_CHECK_POS(n_samples);
  FH_CHECK_POS(U);
  FH_CHECK_POS(n_frames);
  FH_CHECK_POS(hop);
  if (n_fft < 2 || n_fft > FHVAE_FEATS_MAX_NFFT) return FHVAE_ERR_LIMIT;
  if (fbank && (n_mels < 1 || n_mels > FHVAE_FEATS_MAX_NMELS)) return FHVAE_ERR_LIMIT;
  if (hop > 0x7fffffffLL) return FHVAE_ERR_LIMIT;
  if ((((uintptr_t)dft_basis) & 15) != 0 || (fbank && (((uintptr_t)mel_basis) & 15) != 0)) return FHVAE_ERR_ALIGN;
  const int tm = feats_tm(n_fft, fbank);
  if (tm == 0) return FHVAE_ERR_LIMIT;  // fbank above FHVAE_FEATS_MAX_NFFT_FBANK: the tile does not fit in LDS
  FH_CHECK_I32(fh_cdiv(n_frames, 16));
  FH_CHECK_I32(fh_cdiv(U, 256));
  const int n_out = fbank ? (int)n_mels : (int)(n_fft / 2 + 1);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(feats_check_kernel, dim3((unsigned)fh_cdiv(U, 256)), dim3(256), 0, s, wave_ptr, frame_ptr, U, n_samples,
                     n_frames, n_fft, hop, status);
  int rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  return FeatTm::dispatch(tm, [&](auto tmc) {
    constexpr int TM = decltype(tmc)::value;
    return launch_lds(fbank ? feats_kernel<TM, true> : feats_kernel<TM, false>, fh_cdiv(n_frames, 16 * TM), kFeatThreads,
                      feats_smem(16 * TM, n_fft, fbank), s, wave, wave_ptr, frame_ptr, U, n_samples, n_frames, dft_basis,
                      fbank ? mel_basis : nullptr, (int)n_fft, (int)hop, n_out, out, status);
  });
}
