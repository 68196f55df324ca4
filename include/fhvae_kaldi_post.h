/*
 * fhvae_kaldi_post.h -- what Kaldi's recipes put behind the mel bank and in front of a recogniser, on the device
 * (csrc/kaldi_post.hip): cepstra from log-mel rows (the second half of compute-mfcc-feats), delta features (add-deltas)
 * and sliding-window cepstral mean / variance normalisation (apply-cmvn-sliding).  The entry points are exported from the
 * same library as include/fhvae_hip.h and follow its conventions (device pointers, enqueue only, FHVAE_ERR_* before any
 * launch); they are declared here, not there, so FHVAE_ABI_VERSION and the symbol set of that header are unchanged.
 *
 * The definitions below are this project's reading of Kaldi (ComputeDctMatrix, ComputeLifterCoeffs, DeltaFeatures,
 * SlidingWindowCmn), written down: nothing here runs a Kaldi binary, and none was available to compare with.
 *
 * Batch layout (that of fhvae_kaldi_fbank_fwd): the rows of all utterances stacked, frame_ptr (U + 1) int64 on the device
 * their offsets, frame_ptr[0] = 0, frame_ptr[U] = n, not decreasing: the rows of utterance u are frame_ptr[u] ..
 * frame_ptr[u + 1] - 1, T_u = frame_ptr[u + 1] - frame_ptr[u] of them; an utterance with no row is legal.  Every matrix is
 * f32, row-major and, unless a leading dimension is named, contiguous.
 *
 * Cepstra.  dct (C, B): row 0 is sqrt(1 / B), row k is sqrt(2 / B) cos(pi / B (j + 0.5) k), j the bin; lifter (C):
 *   1 + 0.5 Q sin(pi k / Q).  The host computes both in float64 and rounds once (kaldi_post.dct_matrix / lifter_coeffs).
 *     c[f][k]   = fmaf(dct[k][B-1], m[f][B-1], ... fmaf(dct[k][1], m[f][1], fmaf(dct[k][0], m[f][0], 0)))      (f32)
 *     out[f][k] = lifter[k] * c[f][k]   (one f32 product; c[f][k] itself without a lifter)
 *     out[f][0] = max(energy[f], log_energy_floor)   when energy is given (a floor of -inf: none)
 *   The sum is one f32 chain over the bins in increasing order, every step a fused multiply-add, so a row's result depends on
 *   that row alone: bitwise the same alone and in any batch.
 *
 * Deltas.  scales: the order + 1 vectors scales_0 .. scales_order one behind the other, scales_i of 2 i w + 1 values
 *   (w = window): scales_0 = [1], scales_i[m] = (1 / sum_{j=-w..w} j^2) * sum_{j=-w..w} j * scales_{i-1}[m - j] with both
 *   vectors indexed from their centres (m in [-i w, i w]; outside its range scales_{i-1} is 0): the full convolution of
 *   scales_{i-1} with [-w .. w] / sum j^2; built on the host in float64 and rounded once (kaldi_post.delta_scales).  w = 2: [-.2, -.1, 0, .1, .2] and
 *   [.04, .04, .01, -.04, -.1, -.04, .01, .04, .04].  With t the row's index inside its utterance of T rows:
 *     out[f][0 .. D)            = in[f][.]                                                             (a copy, bitwise)
 *     out[f][i D + d], i >= 1   = fmaf(s_i[2iw], x(t + iw), ... fmaf(s_i[1], x(t - iw + 1), fmaf(s_i[0], x(t - iw), 0)))
 *     x(t') = in[frame_ptr[u] + clamp(t', 0, T - 1)][d]
 *   an f32 chain in increasing tap order from 0; the edge row is repeated inside the utterance, never across frame_ptr.  An
 *   utterance's rows are bitwise the same alone or in any batch.
 *
 * Sliding CMVN.  The window [b, e) of frame t of an utterance of T frames, in this order (integer arithmetic):
 *     center:  b = t - cmn_window / 2, e = b + cmn_window          else:  b = t - cmn_window, e = t + 1
 *     if b < 0:                 e -= b; b = 0
 *     if not center and e > t:  e = max(t + 1, min_window)
 *     if e > T:                 b -= e - T; e = T; b = max(b, 0)
 *   (center and cmn_window >= 2 T: b = 0, e = T, per-utterance CMVN.)  Sums are float64 in a fixed two-level order.  The
 *   utterance is cut into chunks of FHVAE_KPOST_CHUNK frames counted from its own first frame; for column d
 *     Q_c(r)  = (((0 + x[c C + 0]) + x[c C + 1]) + ... + x[c C + r - 1])      the first r rows of chunk c, in row order
 *     tot_c   = Q_c(rows of chunk c)
 *     P_c     = (((0 + tot_0) + tot_1) + ... + tot_{c-1})                     the chunks in front, in chunk order
 *     S(t)    = P_c + Q_c(t - c C),  c = t / C                               (t = T with T a multiple of C: P_{T/C} + 0)
 *   and the same with (double)x * (double)x (exact) for the squares, S2.  Then, N = e - b:
 *     mean = (S(e) - S(b)) / N
 *     without norm_vars:  out = (float)((double)x - mean)
 *     with norm_vars:     var = max((S2(e) - S2(b)) / N - mean * mean, 1e-10), var = 1 when N = 1;
 *                         out = (float)(((double)x - mean) * (1 / sqrt(var)))
 *   every operation rounded once (no contraction); float64 division and square root on the device are correctly rounded.
 *   Everything is a function of the utterance alone: bitwise the same alone or in any batch, and a long utterance is
 *   spread over as many workgroups as it has chunks.
 *
 * Status: *status is an int32 device word the library only ORs bits into; the caller clears it.  A frame_ptr that breaks the
 * rules above sets FHVAE_KPOST_BAD_PTR (a check kernel in front) and nothing is written.  The kernels re-check the
 * utterance of every row they touch, so no argument makes a kernel read or write outside its buffers.  No floating-point
 * atomics anywhere.
 */
#ifndef FHVAE_KALDI_POST_H
#define FHVAE_KALDI_POST_H

#include "fhvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { FHVAE_KPOST_BAD_PTR = 1 }; /* frame_ptr does not start at 0, end at n, or decreases */

#define FHVAE_KPOST_MAX_BINS 128   /* B above it: FHVAE_ERR_LIMIT */
#define FHVAE_KPOST_MAX_WINDOW 8   /* delta window above it: FHVAE_ERR_LIMIT */
#define FHVAE_KPOST_MAX_COLS 1024  /* (order + 1) * D of the deltas, D of the CMVN above it: FHVAE_ERR_LIMIT */
#define FHVAE_KPOST_CHUNK 256      /* frames per chunk of the CMVN's prefix sums */

/* out (n, C) from logmel (n, B) with leading dimension ld >= B.  1 <= C <= B (FHVAE_ERR_SHAPE) <= FHVAE_KPOST_MAX_BINS
 * (FHVAE_ERR_LIMIT).  lifter (C) and energy (n) may be NULL.  n == 0: returns 0, launches nothing. */
int fhvae_kaldi_cepstra(const float* logmel, int64_t ld, int64_t n, int64_t B, const float* dct, int64_t C, const float* lifter,
                        const float* energy, float log_energy_floor, float* out, void* stream);

/* out (n, (order + 1) D) from in (n, D).  order in {1, 2} and window >= 1 (FHVAE_ERR_SHAPE), window <=
 * FHVAE_KPOST_MAX_WINDOW and (order + 1) D <= FHVAE_KPOST_MAX_COLS (FHVAE_ERR_LIMIT).  scales: the 1 + (2 w + 1)
 * [+ (4 w + 1)] values above, on the device.  n == 0: returns 0, launches nothing. */
int fhvae_kaldi_add_deltas(const float* in, const int64_t* frame_ptr, int64_t U, int64_t n, int64_t D, int64_t order,
                           int64_t window, const float* scales, float* out, int32_t* status, void* stream);

/* Bytes of the workspace fhvae_kaldi_cmvn_sliding needs for n frames of D columns in U utterances (the chunk totals and
 * their prefixes); < 0: FHVAE_ERR_* for negative sizes or D outside [1, FHVAE_KPOST_MAX_COLS]. */
int64_t fhvae_kaldi_post_ws_bytes(int64_t n, int64_t U, int64_t D);

/* out (n, D) from in (n, D); out may not alias in.  cmn_window >= 1, min_window >= 1, center and norm_vars 0 or 1
 * (FHVAE_ERR_SHAPE); D <= FHVAE_KPOST_MAX_COLS, the windows below 2^31 (FHVAE_ERR_LIMIT).  ws: ws_bytes >=
 * fhvae_kaldi_post_ws_bytes(n, U, D) bytes, 8-byte aligned (FHVAE_ERR_SHAPE / FHVAE_ERR_ALIGN); its contents before and
 * after the call mean nothing.  n == 0: returns 0, launches nothing. */
int fhvae_kaldi_cmvn_sliding(const float* in, const int64_t* frame_ptr, int64_t U, int64_t n, int64_t D, int64_t cmn_window,
                             int64_t min_window, int center, int norm_vars, void* ws, int64_t ws_bytes, float* out,
                             int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
