// resample.hip -- sample-rate conversion of a batch of utterances in one call: librosa.load's resampling (resampy 0.2.2
// kaiser_best through librosa 0.8.0 resample(fix=True, scale=False); the reference's prepare_numpy_data.py:108).
//
// For a rational ratio L / M = sr_out / sr_in the filter has L phases, so the host computes every weight once in float64
// (features.ResampleBank) and the device runs a polyphase FIR as a dense product on the exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32).  An output row is P periods: P * L outputs from the window x[row * P * M - WL + k], k < KP:
//   Y (rows x P*L) = X (rows x KP) . bank^T (KP x NCP)
// A workgroup takes BM = 16 * TM consecutive rows (a tile may span utterances; each row finds its utterance by binary
// search in row_ptr) and gathers their windows into LDS, zero-filled outside the utterance: nothing of a neighbour leaks in
// and the ends are resampy's (no reflection).  Each wave owns whole 16-column groups of the bank for all BM rows, reads the
// bank from L2 straight into registers one 16-k chunk ahead (audio_tile.h) and multiplies only the chunks [c0, c1) in which
// its 16 columns have weights: the bank is banded, the rest of the window would add exact zeros.
//
// resampy advances its time register by repeated float64 addition, and its truncated index_step makes the filter
// discontinuous at integer input times when downsampling.  At the output samples p * L whose register fell just below
// p * M (the host finds them: `exc`), resampy reads the end of the previous interval; a second small kernel recomputes
// those samples with the `alt` weights, one wave per row, lanes strided over the taps and a butterfly sum.
//
// Every output is a fixed-order pair of f32 chains over its own window (each wing towards the centre: chunk, k-step, lane
// group, the MFMA order; then their sum; or lane stride, then butterfly), so an utterance's result does not depend on its
// batch or its place in it: bitwise.  No atomics except the status word's atomicOr.
//
// Pointer errors: a check kernel validates in_ptr / out_ptr / row_ptr against the length rule and sets
// FHVAE_RESAMPLE_BAD_PTR; the other kernels then write nothing.  They also re-check the utterance of every row, so no
// input makes them read or write out of bounds.
#include "audio_tile.h"

namespace fh {

constexpr int kRsThreads = 256;  // 4 waves
using RsTm = TmSet<4, 2, 1>;

// librosa's length rule in float64: resampy computes (int64)(n * ratio) samples, librosa returns ceil(n * ratio)
__host__ __device__ inline int64_t rs_out_len(int64_t n, double ratio) { return (int64_t)__builtin_ceil((double)n * ratio); }
__host__ __device__ inline int64_t rs_calc_len(int64_t n, double ratio) { return (int64_t)((double)n * ratio); }

struct RsRow {
  int64_t in0, n_in, start, out0;  // utterance's first sample and length; window start (utterance coordinates); first output
  int n_out, n_calc;               // outputs of this row to write; of those, computed ones (the rest are the zero tail)
  int64_t p0;                      // first period of the row within its utterance
};

__device__ inline bool rs_find_row(int64_t row, const int64_t* __restrict__ in_ptr, const int64_t* __restrict__ out_ptr,
                                   const int64_t* __restrict__ row_ptr, int64_t U, int64_t n_in_total, int64_t n_out_total,
                                   int64_t n_rows, int64_t PL, int64_t PM, int64_t P, int64_t WL, double ratio, RsRow& r) {
  if (row >= n_rows) return false;
  const int64_t lo = last_le(row_ptr, U, row);
  const int64_t i0 = in_ptr[lo], i1 = in_ptr[lo + 1], o0 = out_ptr[lo], o1 = out_ptr[lo + 1], r0 = row_ptr[lo], r1 = row_ptr[lo + 1];
  const int64_t n = i1 - i0, m = o1 - o0;
  if (!(i0 >= 0 && i1 <= n_in_total && n >= 0 && o0 >= 0 && o1 <= n_out_total && m == rs_out_len(n, ratio) && r0 <= row &&
        row < r1 && r1 - r0 == (m + PL - 1) / PL))
    return false;
  const int64_t rl = row - r0, calc = rs_calc_len(n, ratio);
  r.in0 = i0;
  r.n_in = n;
  r.start = rl * PM - WL;
  r.out0 = o0 + rl * PL;
  const int64_t left = m - rl * PL, cl = calc - rl * PL;
  r.n_out = (int)(left < PL ? left : PL);
  r.n_calc = (int)(cl < 0 ? 0 : cl < r.n_out ? cl : r.n_out);
  r.p0 = rl * P;
  return true;
}

// one thread per utterance
__global__ void resample_check_kernel(const int64_t* __restrict__ in_ptr, const int64_t* __restrict__ out_ptr,
                                      const int64_t* __restrict__ row_ptr, int64_t U, int64_t n_in_total, int64_t n_out_total,
                                      int64_t n_rows, int64_t PL, double ratio, int32_t* status) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const int64_t i0 = in_ptr[u], i1 = in_ptr[u + 1], o0 = out_ptr[u], o1 = out_ptr[u + 1], r0 = row_ptr[u], r1 = row_ptr[u + 1];
  bool ok = i0 >= 0 && i1 >= i0 && i1 <= n_in_total && o0 >= 0 && o1 <= n_out_total && r0 >= 0 && r1 <= n_rows;
  ok = ok && o1 - o0 == rs_out_len(i1 - i0, ratio) && r1 - r0 == (o1 - o0 + PL - 1) / PL;
  if (u == 0) ok = ok && o0 == 0 && r0 == 0;
  if (u == U - 1) ok = ok && o1 == n_out_total && r1 == n_rows;
  if (!ok) atomicOr(status, FHVAE_RESAMPLE_BAD_PTR);
}

// LDS: windows [BM][LDA], LDA = KP + 4 (row stride an odd multiple of 16 bytes: the 16 rows of a ds_read_b128 fragment hit
// 16 distinct bank slots)
template <int TM>
__global__ void __launch_bounds__(kRsThreads) resample_kernel(const float* __restrict__ wave, const int64_t* __restrict__ in_ptr,
                                                              const int64_t* __restrict__ out_ptr, const int64_t* __restrict__ row_ptr,
                                                              int64_t U, int64_t n_in_total, int64_t n_out_total, int64_t n_rows,
                                                              const float* __restrict__ bank, const int32_t* __restrict__ chunks,
                                                              int L, int M, int P, int KP, int WL, double ratio,
                                                              float* __restrict__ out, const int32_t* status) {
  constexpr int BM = 16 * TM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ RsRow rows[BM];  // (with row_ok at most 64 * 52 bytes: the 3.25 KiB FHVAE_RESAMPLE_LDS_FLOATS leaves free)
  __shared__ int row_ok[BM];
  if (*status & FHVAE_RESAMPLE_BAD_PTR) return;
  const int LDA = KP + 4, PL = P * L, G = (PL + 15) / 16, NC = KP / 16;
  float* A = (float*)smem;
  const int tid = threadIdx.x, lane = tid & 63, wave_id = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * BM;

  if (tid < BM) {
    RsRow r = {};
    row_ok[tid] = rs_find_row(row0 + tid, in_ptr, out_ptr, row_ptr, U, n_in_total, n_out_total, n_rows, PL, (int64_t)P * M, P,
                              WL, ratio, r);
    rows[tid] = r;
  }
  __syncthreads();

  // gather: A[r][k] = x[start_r + k] inside the utterance, 0 outside
  for (int e = tid; e < BM * KP; e += kRsThreads) {
    const int r = e / KP, k = e - r * KP;
    float v = 0.f;
    if (row_ok[r]) {
      const int64_t p = rows[r].start + k;
      if (p >= 0 && p < rows[r].n_in) v = wave[rows[r].in0 + p];
    }
    A[r * LDA + k] = v;
  }
  __syncthreads();

  // wave w takes column groups w, w + 4, ...
  for (int g = wave_id; g < G; g += 4) {
    int c0 = chunks[2 * g], c1 = chunks[2 * g + 1];
    c0 = c0 < 0 ? 0 : c0;
    c1 = c1 > NC ? NC : c1;
    // two chains per output, both running from a wing of the filter towards its centre (the left half of the chunks
    // upwards, the right half downwards) and added at the end: the partial sums stay small until the last steps, so the
    // additions round at the size of the wings' terms instead of the result's.
    f32x4 accl[1][TM] = {}, accr[1][TM] = {};
    if (c0 < c1) {
      const float* const br[1] = {bank + (int64_t)(16 * g + i) * KP + 4 * q};
      const float* ar = A + i * LDA + 4 * q;
      const int mid = (c0 + c1 + 1) >> 1;
      tile_product<TM, 1>(accl, br, ar, LDA, c0, mid, 1);
      if (mid < c1) tile_product<TM, 1>(accr, br, ar, LDA, c1 - 1, mid - 1, -1);
#pragma unroll
      for (int t = 0; t < TM; ++t) accl[0][t] += accr[0][t];
    }
    const auto& acc = accl[0];
    // lane (i, q): columns 16g + 4q + v of tile row 16t + i
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      const int r = 16 * t + i;
      if (!row_ok[r]) continue;
      float* o = out + rows[r].out0;
      const int n_out = rows[r].n_out, n_calc = rows[r].n_calc;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int col = 16 * g + 4 * q + v;
        if (col < n_out) o[col] = col < n_calc ? acc[t][v] : 0.f;  // librosa's zero tail past resampy's int(n * ratio)
      }
    }
  }
}

// one wave per row: the outputs p * L of its periods whose time register fell below p * M (exc[p] != 0)
__global__ void __launch_bounds__(64) resample_fix_kernel(const float* __restrict__ wave, const int64_t* __restrict__ in_ptr,
                                                          const int64_t* __restrict__ out_ptr, const int64_t* __restrict__ row_ptr,
                                                          int64_t U, int64_t n_in_total, int64_t n_out_total, int64_t n_rows,
                                                          const uint8_t* __restrict__ exc, int64_t n_exc,
                                                          const float* __restrict__ alt, int alt_taps, int alt_wl, int L, int M,
                                                          int P, int WL, double ratio, float* __restrict__ out,
                                                          const int32_t* status) {
  if (*status & FHVAE_RESAMPLE_BAD_PTR) return;
  RsRow r;
  if (!rs_find_row(blockIdx.x, in_ptr, out_ptr, row_ptr, U, n_in_total, n_out_total, n_rows, (int64_t)P * L, (int64_t)P * M, P,
                   WL, ratio, r))
    return;
  const int lane = threadIdx.x;
  const float* x = wave + r.in0;
  for (int pp = 0; pp < P; ++pp) {
    const int64_t p = r.p0 + pp;
    if (pp * L >= r.n_calc) break;
    if (p >= n_exc || !exc[p]) continue;  // (uniform over the wave)
    const int64_t s0 = p * M - 1 - alt_wl;
    float a = 0.f;
    for (int k = lane; k < alt_taps; k += 64) {
      const int64_t s = s0 + k;
      const float xv = (s >= 0 && s < r.n_in) ? x[s] : 0.f;
      a = __builtin_fmaf(alt[k], xv, a);
    }
    a = wave_sum(a);
    if (lane == 0) out[r.out0 + pp * L] = a;
  }
}

static inline int64_t rs_smem(int BM, int64_t KP) { return (int64_t)BM * 4 * (KP + 4); }

static inline int rs_tm(int64_t KP) {
  return RsTm::largest((int64_t)4 * FHVAE_RESAMPLE_LDS_FLOATS, [&](int BM) { return rs_smem(BM, KP); });
}

}  // namespace fh

using namespace fh;

extern "C" int fhvae_resample_tile_rows(int64_t KP) {
  if (KP < 16 || (KP & 15) != 0) return 0;
  return 16 * rs_tm(KP);
}

extern "C" int fhvae_resample_fwd(const float* wave_in, int64_t n_in, const int64_t* in_ptr, const int64_t* out_ptr,
                                  const int64_t* row_ptr, int64_t U, int64_t n_rows, const float* bank, const int32_t* chunks,
                                  int64_t L, int64_t M, int64_t P, int64_t KP, int64_t WL, double ratio, const uint8_t* exc,
                                  int64_t n_exc, const float* alt, int64_t alt_taps, int64_t alt_wl, float* wave_out,
                                  int64_t n_out, int32_t* status, void* stream) {
  FH_CHECK_PTR(wave_in);
  FH_CHECK_PTR(in_ptr);
  FH_CHECK_PTR(out_ptr);
  FH_CHECK_PTR(row_ptr);
  FH_CHECK_PTR(bank);
  FH_CHECK_PTR(chunks);
  FH_CHECK_PTR(wave_out);
  FH_CHECK_PTR(status);
  FH_CHECK_POS(n_in);
  FH_CHECK_POS(n_out);
  FH_CHECK_POS(n_rows);
  FH_CHECK_POS(U);
  FH_CHECK_POS(L);
  FH_CHECK_POS(M);
  FH_CHECK_POS(P);
  if (!(ratio > 0.0) || WL < 0 || KP < 16 || (KP & 15) != 0) return FHVAE_ERR_SHAPE;
  if (L > FHVAE_RESAMPLE_MAX_L || M > 0x7fffffLL || P > 0x7fffffLL || P * L > 0x7fffffLL || P * M > 0x7fffffLL ||
      WL > 0x7fffffLL)
    return FHVAE_ERR_LIMIT;
  const int64_t NCP = (P * L + 15) / 16 * 16;
  if (NCP * KP > FHVAE_RESAMPLE_MAX_BANK) return FHVAE_ERR_LIMIT;
  const int tm = rs_tm(KP);
  if (tm == 0) return FHVAE_ERR_LIMIT;  // 16 windows do not fit in LDS
  if ((((uintptr_t)bank) & 15) != 0) return FHVAE_ERR_ALIGN;
  if (n_exc < 0 || (n_exc > 0 && (exc == nullptr || alt == nullptr || alt_taps < 1 || alt_taps > 0x7fffffLL || alt_wl < 0 ||
                                  alt_wl > 0x7fffffLL)))
    return n_exc < 0 ? FHVAE_ERR_SHAPE : FHVAE_ERR_NULL;
  FH_CHECK_I32(n_rows);
  FH_CHECK_I32(fh_cdiv(U, 256));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(resample_check_kernel, dim3((unsigned)fh_cdiv(U, 256)), dim3(256), 0, s, in_ptr, out_ptr, row_ptr, U, n_in,
                     n_out, n_rows, P * L, ratio, status);
  int rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  const int l = (int)L, m = (int)M, p = (int)P, kp = (int)KP, wl = (int)WL;
  rc = RsTm::dispatch(tm, [&](auto tmc) {
    constexpr int TM = decltype(tmc)::value;
    return launch_lds(resample_kernel<TM>, fh_cdiv(n_rows, 16 * TM), kRsThreads, rs_smem(16 * TM, KP), s, wave_in, in_ptr, out_ptr,
                      row_ptr, U, n_in, n_out, n_rows, bank, chunks, l, m, p, kp, wl, ratio, wave_out, status);
  });
  if (rc != FHVAE_OK || n_exc == 0) return rc;
  hipLaunchKernelGGL(resample_fix_kernel, dim3((unsigned)n_rows), dim3(64), 0, s, wave_in, in_ptr, out_ptr, row_ptr, U, n_in, n_out,
                     n_rows, exc, n_exc, alt, (int)alt_taps, (int)alt_wl, l, m, p, wl, ratio, wave_out, status);
  return fh_launch_status();
}
