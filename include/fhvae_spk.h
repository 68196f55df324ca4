/*
 * fhvae_spk.h -- the speaker back end on embeddings (csrc/spk.hip): the row transform of a trained LDA / PLDA model and the
 * PLDA log-likelihood ratio of all pairs of rows (its range, its two-class histogram) or of a list of trials.  The entry points
 * are exported from the same library as include/fhvae_hip.h and follow its conventions (device pointers, enqueue only,
 * FHVAE_ERR_* before any launch); they are declared here, not there, so FHVAE_ABI_VERSION and the symbol set of that header
 * are unchanged.  The model itself (centring, LDA, length normalisation, a two-covariance PLDA and its simultaneous
 * diagonalisation) is trained on the host in float64 (spk_backend.py); these calls take its f32 tables.
 *
 * The definitions below are this project's; no Kaldi binary was available to compare with.
 *
 * THE TRANSFORM (fhvae_spk_project), one stage per call, a pure function of the row.  x (S, Din) f32 with leading dimension
 * ldx, A (K, Din) f32 with leading dimension lda, mean (Din); optional q (K) and scale (K); out (S, ldo) f32, a (S) f32.
 *     t_d  = x[d] - mean[d]                                   (f32, rounded once)
 *     y_k  = the chain acc = fmaf(A[k][d], t_d, acc) over d = 0 .. Din - 1 from acc = 0
 *   if normalise != 0:
 *     n    = sqrtf(the chain acc = fmaf(y_k, y_k, acc) over k = 0 .. K - 1 from 0)
 *     r    = sqrtf((float)K) / fmaxf(n, 1e-30f)               (square roots and division correctly rounded)
 *     y_k  = y_k * r                                          (rounded once)
 *   if q is given:
 *     a    = -(the chain acc = fmaf(q[k], y_k * y_k, acc) over k from 0), the square rounded once
 *   out_k  = scale[k] * y_k if scale is given, else y_k;  out_k = 0 for k = K .. ldo - 1
 *   a is written if and only if q is given.  A row's result is bitwise the same alone, in any batch and at any place of a
 *   workgroup: one thread owns a row and nothing is shared between rows.
 *
 * THE SCORE.  v (S, D) f32 with leading dimension ld under the rules of the all-pairs pass (D a multiple of 16 in [16, 128],
 * zero-padded; ld a multiple of 4 and at least D; a 16-byte aligned pointer), a (S) f32, c f32, S <= 2^24:
 *     s(i, j) = (dot(i, j) + (a[i] + a[j])) + c               (one rounding per addition)
 *   With v = sqrt(p) u and a = -sum_k q_k u_k^2 of a diagonalised two-covariance PLDA (within-class covariance I, between-class
 *   covariance diag(psi), p = psi / (2 psi + 1), q = psi^2 / (2 (psi + 1)(2 psi + 1)), c = 1/2 sum_k [2 log(1 + psi_k) -
 *   log(1 + 2 psi_k)]) this is the log-likelihood ratio of "same speaker" against "different speakers" for one row each.
 *   In fhvae_spk_llr_range and fhvae_spk_llr_hist, dot is the all-pairs pass's (csrc/allpairs_f32.h, in its documented order),
 *   which is symmetric bit for bit; a[i] + a[j] commutes: s(i, j) == s(j, i) bit for bit.  A trial is a pair i < j with
 *   label[i] >= 0 and label[j] >= 0; it is a target (class 0) when the labels are equal, else a non-target (class 1).  A trial
 *   whose score is NaN is in neither class and sets FHVAE_SPK_NAN.
 *
 *   fhvae_spk_llr_range: range (2, 2) f32 = per class the minimum and the maximum of s; a class without a trial gives
 *   (+inf, -inf).  Minimum and maximum are taken in the total order of the f32 bit patterns (-0 below +0): no order of arrival
 *   and no grid changes a bit of the result.
 *
 *   fhvae_spk_llr_hist: hist (2, NB) uint64, NB a power of two in [64, 8192]; lo <= hi, both finite.
 *     scale = (float)NB / (hi - lo), or 0 when hi == lo        (f32)
 *     bin   = clamp(floorf((s - lo) * scale), 0, NB - 1)       (a product that is NaN -- an infinite s with scale 0 -- goes to bin 0)
 *     hist[class][bin] += 1
 *   Counts are integers: the result does not depend on the grid or on the order of arrival.
 *
 *   fhvae_spk_llr_trials: pairs (n, 2) int32, out (n) f32.  dot is the chain acc = fmaf(v[i][d], v[j][d], acc) over d = 0 ..
 *   D - 1 from 0, then the same two additions: (i, j) and (j, i) give the same bits, and i == j is scored like any pair.  An
 *   index outside [0, S) sets FHVAE_SPK_BAD_INDEX and that score is NaN; every index is checked before it is used.  (The chain
 *   meets the columns in another order than the all-pairs dot: a trial's score and the all-pairs score of the same rows differ
 *   by rounding.)
 *
 * Status: *status is an int32 device word the library only ORs bits into; the caller clears it.
 */
#ifndef FHVAE_SPK_H
#define FHVAE_SPK_H

#include "fhvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  FHVAE_SPK_NAN = 1,      /* a trial's score is NaN: it is counted in neither class */
  FHVAE_SPK_BAD_INDEX = 2 /* a pair names a row outside [0, S): its score is NaN */
};

#define FHVAE_SPK_MAX_IN 1024     /* Din above it: FHVAE_ERR_LIMIT */
#define FHVAE_SPK_MAX_ROWS 16777216 /* S above 2^24: FHVAE_ERR_LIMIT */

/* bytes of workspace of fhvae_spk_llr_range; 0 for arguments the calls below refuse.  Monotone in each argument. */
int64_t fhvae_spk_ws_bytes(int64_t S, int64_t D);

/* S, Din, K < 1, K > 128, ldx or lda below Din, ldo below K or no multiple of 4: FHVAE_ERR_SHAPE; x, A, mean, q, scale or a off
 * 4 bytes, out off 16 bytes: FHVAE_ERR_ALIGN; Din above FHVAE_SPK_MAX_IN or S above FHVAE_SPK_MAX_ROWS: FHVAE_ERR_LIMIT.  q and a
 * are given together or not at all (else FHVAE_ERR_NULL); scale may be NULL. */
int fhvae_spk_project(const float* x, int64_t ldx, int64_t S, int64_t Din, const float* A, int64_t lda, int64_t K, const float* mean,
                      int normalise, const float* q, const float* scale, float* out, int64_t ldo, float* a, void* stream);

/* ws: fhvae_spk_ws_bytes(S, D) bytes, 4-byte aligned; nothing in it outlives the call.  S < 1, a D or ld the all-pairs pass does
 * not take, ws_bytes too small: FHVAE_ERR_SHAPE; alignment: FHVAE_ERR_ALIGN; S above FHVAE_SPK_MAX_ROWS: FHVAE_ERR_LIMIT. */
int fhvae_spk_llr_range(const float* v, int64_t ld, const float* a, const int32_t* label, int64_t S, int64_t D, float c, void* ws,
                        int64_t ws_bytes, float* range, int32_t* status, void* stream);

/* no workspace; v, ld, a, label, S, D as above; n_bins no power of two in [64, 8192], lo or hi not finite, hi < lo:
 * FHVAE_ERR_SHAPE; hist off 8 bytes: FHVAE_ERR_ALIGN.  hist is zeroed by the call. */
int fhvae_spk_llr_hist(const float* v, int64_t ld, const float* a, const int32_t* label, int64_t S, int64_t D, float c, float lo,
                       float hi, int64_t n_bins, uint64_t* hist, int32_t* status, void* stream);

/* n < 1: FHVAE_ERR_SHAPE; n above 2^31 - 1: FHVAE_ERR_LIMIT; the rest as above */
int fhvae_spk_llr_trials(const float* v, int64_t ld, const float* a, int64_t S, int64_t D, float c, const int32_t* pairs, int64_t n,
                         float* out, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
