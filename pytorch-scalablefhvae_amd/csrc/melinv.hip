// melinv.hip -- linear magnitudes from mel magnitudes, the step csrc/synth.hip lacks for "fbank" features:
//
//   per frame   minimise ||A x - m||^2 over x >= 0,   A = the slaney mel bank (n_mels x n_bins),  m = the frame's mel magnitudes
//
// by a fixed number of accelerated projected-gradient (FISTA) steps from zero, all of them in ONE launch:
//
//   x = y = 0;  repeat n_iter times:  r = A y - m;  g = A^T r;  x+ = max(y - g / L, 0);  y = x+ + beta_k (x+ - x);  x = x+
//
// 1 / L (L = lambda_max(A A^T), nudged up) and the momentum factors beta_k come from the host, which computes them in float64.
//
// The bank is banded: slaney triangles overlap by half, so a bin lies in at most two ADJACENT filters and a filter is one
// contiguous run of bins (391 non-zeros of 16,080 entries at 16 kHz / 80 mels).  The host hands the band over from both sides:
//   per bin b      bin_filt[b] = f, bin_w[2b] = A[f, b], bin_w[2b + 1] = A[f + 1, b]            (for g = A^T r)
//   per filter j   filt_first[j], filt_off[j] .. filt_off[j + 1] into filt_w = A[j, first ...]   (for r = A y - m)
// so an iteration is about 2 * nnz + 4 * n_bins FMAs per frame on the VALU instead of two dense 80 x 201 products.
//
// A workgroup takes a tile of TF frames, one frame per lane (lane-contiguous LDS columns: no bank conflicts), and keeps x, y,
// r and m in LDS for the whole loop; HBM is touched twice, to read m and to write x.  Its threads form P = threads / TF
// parts: in the gradient phase part p sweeps a contiguous range of bins, in the residual phase a contiguous range of
// filters (ranges balanced by non-zeros), with one barrier after each.  With TF = 64 a part is a whole wave, the bin and
// filter indices are wave-uniform and the band's weights arrive by scalar loads.
//
// Every output is a fixed-order f32 chain over values of its own frame (a filter's sum runs over its bins in increasing
// order in one thread, whatever the partition), so a frame's result does not depend on the batch or its place in it: bitwise.
//
// A band that would make the kernel read outside its arrays sets FHVAE_MELINV_BAD_BAND in the status word (a check kernel in
// front); the main kernel then writes nothing.
#include "audio_tile.h"

namespace fh {
namespace {

constexpr float kMiLogFloor = -50.f;  // the "spec" features' floor (csrc/feats.hip)

__global__ void melinv_check_kernel(const int32_t* __restrict__ bin_filt, const int32_t* __restrict__ filt_first,
                                    const int32_t* __restrict__ filt_off, int n_bins, int n_mels, int nnz, int32_t* status) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  bool ok = true;
  if (t < n_bins) {
    const int f = bin_filt[t];
    ok = f >= 0 && f < n_mels;
  }
  if (t < n_mels) {
    const int o0 = filt_off[t], o1 = filt_off[t + 1], first = filt_first[t];
    ok = ok && o0 >= 0 && o1 >= o0 && o1 <= nnz && first >= 0 && first <= n_bins && o1 - o0 <= n_bins - first;
    if (t == 0) ok = ok && o0 == 0;
    if (t == n_mels - 1) ok = ok && o1 == nnz;
  }
  if (!ok) atomicOr(status, FHVAE_MELINV_BAD_BAND);
}

// LDS: X [n_bins][TF], Y [n_bins][TF], R [n_mels][TF], M [n_mels][TF]; thread (part p, frame fr) = tid / TF, tid % TF
template <int TF, int NT>
__global__ void __launch_bounds__(NT) melinv_kernel(const float* __restrict__ mel, int64_t n_frames, int n_mels, int n_bins,
                                                    const int32_t* __restrict__ bin_filt, const float* __restrict__ bin_w,
                                                    const int32_t* __restrict__ filt_first, const int32_t* __restrict__ filt_off,
                                                    const float* __restrict__ filt_w, float inv_l, const float* __restrict__ beta,
                                                    int n_iter, int in_log, int out_log, float* __restrict__ out,
                                                    const int32_t* status) {
  constexpr int P = NT / TF;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if (*status & FHVAE_MELINV_BAD_BAND) return;
  float* X = (float*)smem;
  float* Y = X + n_bins * TF;
  float* R = Y + n_bins * TF;
  float* M = R + n_mels * TF;
  const int tid = threadIdx.x, fr = tid % TF;
  // a part of 64 frames is one wave: tell the compiler, so that everything indexed by bin or filter goes through SGPRs
  const int p = TF == 64 ? __builtin_amdgcn_readfirstlane(tid / TF) : tid / TF;
  const int64_t f0 = (int64_t)blockIdx.x * TF;

  for (int e = tid; e < TF * n_mels; e += NT) {  // (coalesced over the tile's rows of `mel`)
    const int r = e / n_mels, j = e - r * n_mels;
    float v = 0.f;
    if (f0 + r < n_frames) {
      v = mel[(f0 + r) * (int64_t)n_mels + j];
      if (in_log) v = expf(v);
    }
    M[j * TF + r] = v;
    R[j * TF + r] = -v;  // r = A y - m at y = 0
  }
  for (int e = tid; e < 2 * n_bins * TF; e += NT) X[e] = 0.f;  // X and Y

  // the part's bins, and its filters: filter j weighs (its bins + 1), the running weight decides the part
  const int b0 = (int)((int64_t)p * n_bins / P), b1 = (int)((int64_t)(p + 1) * n_bins / P);
  const int64_t total = (int64_t)filt_off[n_mels] + n_mels;
  int j0 = n_mels, j1 = n_mels;
  for (int j = n_mels - 1; j >= 0; --j) {
    const int q = (int)(((int64_t)filt_off[j] + j) * P / total);  // non-decreasing in j, below P
    if (q >= p) j0 = j;
    if (q > p) j1 = j;
  }
  __syncthreads();

  for (int it = 0; it < n_iter; ++it) {
    const float bt = beta[it];
    // gradient step on the part's bins: g = A^T r has at most two terms
#pragma unroll 4
    for (int b = b0; b < b1; ++b) {
      const int fl = bin_filt[b];
      const int fu = fl + 1 < n_mels ? fl + 1 : n_mels - 1;  // (its weight is zero when there is no filter above)
      const float w0 = bin_w[2 * b], w1 = bin_w[2 * b + 1];
      const float g = __builtin_fmaf(w1, R[fu * TF + fr], w0 * R[fl * TF + fr]);
      const float y = Y[b * TF + fr], xo = X[b * TF + fr];
      const float xn = fmaxf(__builtin_fmaf(-inv_l, g, y), 0.f);
      X[b * TF + fr] = xn;
      Y[b * TF + fr] = __builtin_fmaf(bt, xn - xo, xn);
    }
    __syncthreads();
    if (it + 1 == n_iter) break;  // (the last residual is never read)
    // residual of the part's filters: r_j = sum over the filter's run of bins, in increasing order, minus m_j
    for (int j = j0; j < j1; ++j) {
      const int o0 = filt_off[j], o1 = filt_off[j + 1];
      const float* yr = Y + filt_first[j] * TF + fr;
      const float* wr = filt_w + o0;
      float acc = 0.f;
#pragma unroll 4
      for (int k = 0; k < o1 - o0; ++k) acc = __builtin_fmaf(wr[k], yr[k * TF], acc);
      R[j * TF + fr] = acc - M[j * TF + fr];
    }
    __syncthreads();
  }

  for (int e = tid; e < TF * n_bins; e += NT) {  // (coalesced over the tile's rows of `out`)
    const int r = e / n_bins, b = e - r * n_bins;
    if (f0 + r >= n_frames) break;
    float v = X[b * TF + r];
    // (through double: the stored logarithm is the correctly rounded one of the stored magnitude, once per output element)
    if (out_log) v = fmaxf((float)log((double)v), kMiLogFloor);
    out[(f0 + r) * (int64_t)n_bins + b] = v;
  }
}

static inline int64_t melinv_smem(int tf, int64_t n_mels, int64_t n_bins) { return (int64_t)tf * 4 * (2 * n_bins + 2 * n_mels); }

// the widest tile (one frame per lane, at most a wave) whose state fits in LDS
static inline int melinv_tf(int64_t n_mels, int64_t n_bins) {
  for (int tf = 64; tf >= 8; tf >>= 1)
    if (melinv_smem(tf, n_mels, n_bins) <= kCuLdsBytes) return tf;
  return 0;
}

template <int TF, int NT>
static int melinv_launch(const float* mel, int64_t n_frames, int n_mels, int n_bins, const int32_t* bin_filt, const float* bin_w,
                         const int32_t* filt_first, const int32_t* filt_off, const float* filt_w, float inv_l, const float* beta,
                         int n_iter, int flags, float* out, const int32_t* status, hipStream_t s) {
  return launch_lds(melinv_kernel<TF, NT>, fh_cdiv(n_frames, TF), NT, melinv_smem(TF, n_mels, n_bins), s, mel, n_frames, n_mels, n_bins,
                    bin_filt, bin_w, filt_first, filt_off, filt_w, inv_l, beta, n_iter, (flags & FHVAE_MELINV_IN_LOG) != 0,
                    (flags & FHVAE_MELINV_OUT_LOG) != 0, out, status);
}

}  // namespace
}  // namespace fh

using namespace fh;

extern "C" int fhvae_mel_invert_tile_rows(int64_t n_mels, int64_t n_bins) {
  if (n_mels < 1 || n_mels > FHVAE_FEATS_MAX_NMELS || n_bins < 2 || n_bins > FHVAE_FEATS_MAX_NFFT / 2 + 1) return 0;
  return melinv_tf(n_mels, n_bins);
}

extern "C" int fhvae_mel_invert(const float* mel, int64_t n_frames, int64_t n_mels, int64_t n_bins, const int32_t* bin_filt,
                                const float* bin_w, const int32_t* filt_first, const int32_t* filt_off, const float* filt_w,
                                int64_t nnz, float inv_l, const float* beta, int64_t n_iter, int flags, float* out, int32_t* status,
                                void* stream) {
  FH_CHECK_PTR(mel);
  FH_CHECK_PTR(bin_filt);
  FH_CHECK_PTR(bin_w);
  FH_CHECK_PTR(filt_first);
  FH_CHECK_PTR(filt_off);
  FH_CHECK_PTR(beta);
  FH_CHECK_PTR(out);
  FH_CHECK_PTR(status);
  if (nnz > 0) FH_CHECK_PTR(filt_w);
  FH_CHECK_POS(n_frames);
  FH_CHECK_POS(n_iter);
  if (nnz < 0) return FHVAE_ERR_SHAPE;
  if (n_mels < 1 || n_mels > FHVAE_FEATS_MAX_NMELS || n_bins < 2 || n_bins > FHVAE_FEATS_MAX_NFFT / 2 + 1) return FHVAE_ERR_LIMIT;
  if (nnz > 2 * n_bins) return FHVAE_ERR_LIMIT;  // (a bin lies in at most two filters)
  if (!(inv_l > 0.f) || !(inv_l < 3.0e38f)) return FHVAE_ERR_LIMIT;  // (NaN too)
  if (flags & ~(FHVAE_MELINV_IN_LOG | FHVAE_MELINV_OUT_LOG)) return FHVAE_ERR_SHAPE;
  FH_CHECK_I32(n_iter);
  const int tf = melinv_tf(n_mels, n_bins);
  if (tf == 0) return FHVAE_ERR_LIMIT;
  FH_CHECK_I32(fh_cdiv(n_frames, tf));
  hipStream_t s = (hipStream_t)stream;
  const int nm = (int)n_mels, nb = (int)n_bins, ni = (int)n_iter;
  const int most = nm > nb ? nm : nb;
  hipLaunchKernelGGL(melinv_check_kernel, dim3((unsigned)fh_cdiv(most, 256)), dim3(256), 0, s, bin_filt, filt_first, filt_off, nb, nm,
                     (int)nnz, status);
  int rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  if (tf == 64) return melinv_launch<64, 512>(mel, n_frames, nm, nb, bin_filt, bin_w, filt_first, filt_off, filt_w, inv_l, beta, ni, flags, out, status, s);
  if (tf == 32) return melinv_launch<32, 256>(mel, n_frames, nm, nb, bin_filt, bin_w, filt_first, filt_off, filt_w, inv_l, beta, ni, flags, out, status, s);
  if (tf == 16) return melinv_launch<16, 256>(mel, n_frames, nm, nb, bin_filt, bin_w, filt_first, filt_off, filt_w, inv_l, beta, ni, flags, out, status, s);
  return melinv_launch<8, 256>(mel, n_frames, nm, nb, bin_filt, bin_w, filt_first, filt_off, filt_w, inv_l, beta, ni, flags, out, status, s);
}
