// kaldi_fbank.hip -- Kaldi's compute-fbank-feats for a batch of utterances in one launch: snip-edges framing, dither,
// per-frame DC removal, in-frame pre-emphasis, window, P-point power spectrum, HTK mel triangles, log (the features the
// reference gets by shelling out to Kaldi, prepare_kaldi_data.py:38-73).
//
// The scheme of audio_tile.h: a workgroup takes BM = 16*TM consecutive output rows (frames; a tile may span utterances,
// each row finds its utterance by binary search in frame_ptr), gathers them into LDS and runs two dense products
// (tile_product) on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32):
//   DFT:  [c | s] = frame (1 x KP) . basis^T      basis rows = window * cos / -sin of the P-point DFT over the N non-zero
//                                                 columns (host-built, f64 -> f32), bins 0 .. P/2 - 1
//   mel:  M = (c^2 + s^2) (1 x NBP) . mel^T
// The gather differs: a row belongs to one wave.  Pass 1 loads the frame's N samples (a lane owns quads of 4 consecutive
// samples: one Philox4x32-10 block gives their 4 normals), adds the dither noise, writes them to LDS and sums them (lane
// partial sums in quad order, then the xor butterfly: a fixed order).  Pass 2 reads each lane's own quads back, subtracts
// the mean, applies x[i] -= c x[i-1] with the left neighbour from the lane below (__shfl_up; the quad before lane 0's comes
// from the previous 64-quad round) and x[0] -= c x[0], and writes the row in place.
//
// Every output element is a fixed-order f32 chain over its own frame, so a frame's result does not depend on the other
// frames of its launch or its place in the tile: bitwise.  The noise is a function of (seed, stream id of the utterance,
// frame index within the utterance, sample index) alone.
//
// Pointer errors: a check kernel validates wave_ptr / frame_ptr against the framing rule and sets FHVAE_KALDI_BAD_PTR; the
// main kernel then writes nothing.  It also re-checks the utterance of every row it gathers, so no input makes it read or
// write out of bounds.
#include <float.h>

#include "audio_tile.h"

namespace fh {

constexpr int kKfThreads = 256;  // 4 waves
constexpr int kKfMaxBM = 64;
using KfTm = TmSet<4, 3, 2, 1>;

__host__ __device__ inline int64_t kaldi_frames(int64_t L, int64_t N, int64_t S) { return L < N ? 0 : 1 + (L - N) / S; }

// one thread per utterance: monotone pointers, at least one frame, frame counts by the snip-edges rule
__global__ void kaldi_fbank_check_kernel(const int64_t* __restrict__ wave_ptr, const int64_t* __restrict__ frame_ptr, int64_t U,
                                         int64_t n_samples, int64_t n_frames, int64_t N, int64_t S, int32_t* status) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const int64_t w0 = wave_ptr[u], w1 = wave_ptr[u + 1], f0 = frame_ptr[u], f1 = frame_ptr[u + 1];
  bool ok = w0 >= 0 && w1 <= n_samples && w1 - w0 >= N;
  ok = ok && f0 >= 0 && f1 <= n_frames && f1 - f0 == (ok ? kaldi_frames(w1 - w0, N, S) : -1);
  if (u == 0) ok = ok && f0 == 0;
  if (u == U - 1) ok = ok && f1 == n_frames;
  if (!ok) atomicOr(status, FHVAE_KALDI_BAD_PTR);
}

// Philox4x32-10 (Salmon et al. 2011): counter (c0, c1, c2, c3), key (k0, k1) -> four 32-bit words
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c.x), l0 = 0xD2511F53u * c.x;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c.z), l1 = 0xCD9E8D57u * c.z;
    c = make_uint4(h1 ^ c.y ^ k0, l1, h0 ^ c.w ^ k1, l0);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// two words -> two standard normals (Box-Muller); u = ((r >> 9) + 0.5) * 2^-23 is exact in f32 and never 0 or 1
__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& z0, float& z1) {
  const float u1 = (float)(2u * (ra >> 9) + 1u) * 0x1p-24f, u2 = (float)(2u * (rb >> 9) + 1u) * 0x1p-24f;
  const float rad = __builtin_sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincospif(2.0f * u2, &sn, &cs);
  z0 = rad * cs;
  z1 = rad * sn;
}

struct KaldiFbankArgs {
  const float* wave;
  const int64_t* wave_ptr;
  const int64_t* frame_ptr;
  const uint64_t* stream_ids;
  int64_t U, n_samples, n_frames;
  const float* dft;
  const float* melb;
  int N, S, P, n_out, flags;
  float preemph, dither;
  uint64_t seed;
  float* out;
  const int32_t* status;
};

// LDS: frames [BM][LDA] (LDA = KP + 4), then the power (or magnitude) spectrum [BM][LDM] (LDM = NBP + 4)
template <int TM, bool DITHER>
__global__ void __launch_bounds__(kKfThreads) kaldi_fbank_kernel(const KaldiFbankArgs a) {
  constexpr int BM = 16 * TM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int64_t row_src[BM];     // index of the frame's first sample in wave; -1: no such row
  __shared__ uint32_t row_frame[BM];  // frame index within the utterance
  __shared__ uint64_t row_stream[BM];
  if (*a.status & FHVAE_KALDI_BAD_PTR) return;  // (set by the check kernel: the rows would not be unique)
  const int N = a.N, KP = (N + 15) & ~15, LDA = KP + 4;
  const int n_bins = a.P / 2, G = (n_bins + 15) / 16, NBP = 16 * G, LDM = NBP + 4;
  float* A = (float*)smem;
  float* Ms = A + BM * LDA;
  const int tid = threadIdx.x, lane = tid & 63, wave_id = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int64_t f0 = (int64_t)blockIdx.x * BM;

  if (tid < BM) {
    const int64_t f = f0 + tid;
    int64_t src = -1;
    uint32_t fi = 0;
    uint64_t sid = 0;
    if (f < a.n_frames) {
      const int64_t lo = last_le(a.frame_ptr, a.U, f);
      const int64_t w0 = a.wave_ptr[lo], w1 = a.wave_ptr[lo + 1], p0 = a.frame_ptr[lo], p1 = a.frame_ptr[lo + 1];
      const int64_t L = w1 - w0;
      // p1 - p0 == frames(L) and f < p1 keep (f - p0) * S + N <= L: the frame lies inside its utterance
      if (w0 >= 0 && w1 <= a.n_samples && L >= N && p0 <= f && f < p1 && p1 - p0 == kaldi_frames(L, N, a.S)) {
        src = w0 + (f - p0) * a.S;
        fi = (uint32_t)(f - p0);
        if constexpr (DITHER) sid = a.stream_ids[lo];
      }
    }
    row_src[tid] = src;
    row_frame[tid] = fi;
    row_stream[tid] = sid;
  }
  __syncthreads();

  // ---- gather: wave w takes rows w, w + 4, ...; a lane owns the quads lane, lane + 64, ... of the row
  const int NQ = KP / 4;
  const float c = a.preemph;
  for (int r = wave_id; r < BM; r += 4) {
    float* row = A + r * LDA;
    const int64_t src = row_src[r];
    if (src < 0) {
      for (int qd = lane; qd < NQ; qd += 64) *(float4*)(row + 4 * qd) = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    const float* y = a.wave + src;
    float part = 0.f;
    for (int qd = lane; qd < NQ; qd += 64) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = 4 * qd + e < N ? y[4 * qd + e] : 0.f;
      if constexpr (DITHER) {
        const uint64_t sid = row_stream[r];
        const uint4 rnd = philox4x32_10(make_uint4(row_frame[r], (uint32_t)qd, (uint32_t)sid, (uint32_t)(sid >> 32)),
                                        (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
        float z[4];
        box_muller(rnd.x, rnd.y, z[0], z[1]);
        box_muller(rnd.z, rnd.w, z[2], z[3]);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = 4 * qd + e < N ? __builtin_fmaf(a.dither, z[e], v[e]) : 0.f;
      }
      part += (v[0] + v[1]) + (v[2] + v[3]);
      *(float4*)(row + 4 * qd) = make_float4(v[0], v[1], v[2], v[3]);
    }
    const float mean = (a.flags & FHVAE_KALDI_REMOVE_DC) ? wave_sum(part) / (float)N : 0.f;
    float carry = 0.f;  // the last sample of the previous round of 64 quads
    for (int base = 0; base < NQ; base += 64) {
      const int qd = base + lane;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (qd < NQ) {
        const float4 t = *(const float4*)(row + 4 * qd);  // this lane's own write of pass 1
        v[0] = t.x - mean; v[1] = t.y - mean; v[2] = t.z - mean; v[3] = t.w - mean;
      }
      float prev = __shfl_up(v[3], 1, 64);
      if (lane == 0) prev = base == 0 ? v[0] : carry;  // x[0] -= c x[0]
      carry = __shfl(v[3], 63, 64);
      if (qd < NQ) {
        float o[4];
        o[0] = __builtin_fmaf(-c, prev, v[0]);
#pragma unroll
        for (int e = 1; e < 4; ++e) o[e] = __builtin_fmaf(-c, v[e - 1], v[e]);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = 4 * qd + e < N ? o[e] : 0.f;
        *(float4*)(row + 4 * qd) = make_float4(o[0], o[1], o[2], o[3]);
      }
    }
  }
  __syncthreads();

  const int NC = KP / 16;
  // ---- DFT: wave w takes bin groups w, w+4, ...
  for (int g = wave_id; g < G; g += 4) {
    f32x4 acc[2][TM] = {};
    const float* bc = a.dft + (int64_t)(32 * g + i) * KP + 4 * q;
    const float* const bcs[2] = {bc, bc + (int64_t)16 * KP};
    tile_product<TM, 2>(acc, bcs, A + i * LDA + 4 * q, LDA, 0, NC, 1);
    const auto &ac = acc[0], &as = acc[1];
    // lane (i, q): bins 16g + 4q + v of tile row 16t + i (padded bins: zero basis rows -> 0)
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      float m[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        m[v] = __builtin_fmaf(ac[t][v], ac[t][v], as[t][v] * as[t][v]);
        if (!(a.flags & FHVAE_KALDI_USE_POWER)) m[v] = __builtin_sqrtf(m[v]);
      }
      *(float4*)(Ms + (16 * t + i) * LDM + 16 * g + 4 * q) = make_float4(m[0], m[1], m[2], m[3]);
    }
  }
  __syncthreads();

  // ---- mel: M[r][j] = sum over bins of spectrum[r][bin] * mel[j][bin]; wave w takes mel groups w, w+4, ...
  const int H = (a.n_out + 15) / 16, NCM = NBP / 16;
  for (int h = wave_id; h < H; h += 4) {
    f32x4 accm[1][TM] = {};
    const float* const br[1] = {a.melb + (int64_t)(16 * h + i) * NBP + 4 * q};
    tile_product<TM, 1>(accm, br, Ms + i * LDM + 4 * q, LDM, 0, NCM, 1);
    const auto& acc = accm[0];
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      const int r = 16 * t + i;
      if (row_src[r] < 0) continue;
      float* o = a.out + (f0 + r) * (int64_t)a.n_out;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int j = 16 * h + 4 * q + v;
        if (j >= a.n_out) continue;
        const float e = acc[t][v];
        // log(max(e, FLT_EPSILON)); the floor is the f32 nearest to ln 2^-23 whatever logf rounds to
        o[j] = !(a.flags & FHVAE_KALDI_USE_LOG) ? e : e > FLT_EPSILON ? logf(e) : -15.942385152878742f;
      }
    }
  }
}

// LDS bytes of the dynamic part for a BM-row tile
static inline int64_t kf_smem(int BM, int64_t N, int64_t P) {
  const int64_t KP = (N + 15) & ~15LL, NBP = 16 * ((P / 2 + 15) / 16);
  return (int64_t)BM * 4 * ((KP + 4) + (NBP + 4));
}
constexpr int64_t kKfStaticLds = kKfMaxBM * (8 + 4 + 8);

static inline bool kf_sizes_ok(int64_t N, int64_t P) {
  return N >= 2 && P >= N && P < 2 * N && (P & (P - 1)) == 0 && P <= FHVAE_KALDI_MAX_P;
}

static inline int kf_tm(int64_t N, int64_t P) {
  return KfTm::largest(kCuLdsBytes, [&](int BM) { return kf_smem(BM, N, P) + kKfStaticLds; });
}

}  // namespace fh

using namespace fh;

extern "C" int fhvae_kaldi_fbank_tile_rows(int64_t frame_len, int64_t padded_len, int64_t n_mels) {
  if (!kf_sizes_ok(frame_len, padded_len) || n_mels < 1 || n_mels > FHVAE_FEATS_MAX_NMELS) return 0;
  return 16 * kf_tm(frame_len, padded_len);
}

extern "C" int fhvae_kaldi_fbank_fwd(const float* wave, int64_t n_samples, const int64_t* wave_ptr, const int64_t* frame_ptr,
                                     const uint64_t* stream_ids, int64_t U, int64_t n_frames, const float* dft_basis,
                                     const float* mel_basis, int64_t frame_len, int64_t frame_shift, int64_t padded_len,
                                     int64_t n_mels, float preemph, float dither, uint64_t seed, int flags, float* out,
                                     int32_t* status, void* stream) {
  FH_CHECK_PTR(wave);
  FH_CHECK_PTR(wave_ptr);
  FH_CHECK_PTR(frame_ptr);
  FH_CHECK_PTR(dft_basis);
  FH_CHECK_PTR(mel_basis);
  FH_CHECK_PTR(out);
  FH_CHECK_PTR(status);
  const bool dith = dither != 0.f;
  if (dith) FH_CHECK_PTR(stream_ids);
  FH_CHECK_POS(n_samples);
  FH_CHECK_POS(U);
  FH_CHECK_POS(n_frames);
  if (flags & ~(FHVAE_KALDI_REMOVE_DC | FHVAE_KALDI_USE_LOG | FHVAE_KALDI_USE_POWER)) return FHVAE_ERR_SHAPE;
  if (frame_len < 2 || frame_shift < 1 || frame_shift > frame_len) return FHVAE_ERR_SHAPE;
  if (padded_len > FHVAE_KALDI_MAX_P) return FHVAE_ERR_LIMIT;
  if (!kf_sizes_ok(frame_len, padded_len)) return FHVAE_ERR_SHAPE;  // not the smallest power of two >= frame_len
  if (n_mels < 1 || n_mels > FHVAE_FEATS_MAX_NMELS) return FHVAE_ERR_LIMIT;
  if ((((uintptr_t)dft_basis) & 15) != 0 || (((uintptr_t)mel_basis) & 15) != 0) return FHVAE_ERR_ALIGN;
  const int tm = kf_tm(frame_len, padded_len);
  if (tm == 0) return FHVAE_ERR_LIMIT;
  FH_CHECK_I32(fh_cdiv(n_frames, 16));
  FH_CHECK_I32(fh_cdiv(U, 256));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kaldi_fbank_check_kernel, dim3((unsigned)fh_cdiv(U, 256)), dim3(256), 0, s, wave_ptr, frame_ptr, U, n_samples,
                     n_frames, frame_len, frame_shift, status);
  int rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  KaldiFbankArgs a;
  a.wave = wave; a.wave_ptr = wave_ptr; a.frame_ptr = frame_ptr; a.stream_ids = stream_ids;
  a.U = U; a.n_samples = n_samples; a.n_frames = n_frames;
  a.dft = dft_basis; a.melb = mel_basis;
  a.N = (int)frame_len; a.S = (int)frame_shift; a.P = (int)padded_len; a.n_out = (int)n_mels; a.flags = flags;
  a.preemph = preemph; a.dither = dither; a.seed = seed;
  a.out = out; a.status = status;
  return KfTm::dispatch(tm, [&](auto tmc) {
    constexpr int TM = decltype(tmc)::value;
    return launch_lds(dith ? kaldi_fbank_kernel<TM, true> : kaldi_fbank_kernel<TM, false>, fh_cdiv(n_frames, 16 * TM), kKfThreads,
                      kf_smem(16 * TM, frame_len, padded_len), s, a);
  });
}
