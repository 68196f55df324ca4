/*
 * fhvae_snorm.h -- score normalisation against a cohort for the speaker back end (csrc/snorm.hip, csrc/spk.hip): the mean and
 * the standard deviation of the K largest cohort scores of every evaluation row (S-norm with the whole cohort, adaptive S-norm
 * with the top K), and the normalised score of all pairs of rows (its range, its two-class histogram) or of a list of trials.
 * The entry points are exported from the same library as include/fhvae_hip.h and follow its conventions (device pointers,
 * enqueue only, FHVAE_ERR_* before any launch); they are declared here, so FHVAE_ABI_VERSION and the symbol set of that header
 * are unchanged.  The operands are include/fhvae_spk.h's: rows v and a row term a that a back end made (the PLDA's, or rows of
 * unit length with a = 0 and c = 0, whose dot is the cosine).
 *
 * The definitions below are this project's.
 *
 * OPERANDS.  Evaluation rows v (S, D) f32 with leading dimension ld and a (S); cohort rows z (Nc, D) with leading dimension
 * ldz and az (Nc); a scalar c.  D a multiple of 16 in [16, 128], zero-padded; ld and ldz multiples of 4 and at least D; v and z
 * 16-byte aligned (the rules of the all-pairs pass).  S <= 2^24, Nc <= 2^20.
 *
 * THE COHORT SCORE.  s(i, n) = (dot(v_i, z_n) + (a[i] + az[n])) + c, dot the all-pairs pass's (csrc/allpairs_f32.h, in its
 * documented order), one rounding per addition.
 *
 * THE SELECTION.  K = Nc if top <= 0, else min(top, Nc).  T_i is the K-th largest of s(i, .) in the total order of the f32 bit
 * patterns with the sign folded (-0 below +0).  The multiset of the K largest values is unique whatever breaks ties, so nothing
 * below depends on tie-breaking or, up to the rounding of the sums, on the order of the cohort.
 *
 * THE STATISTICS, in float64, over the members n whose score lies above T_i in that order (a tie at the threshold adds d = 0 and
 * needs no count):
 *     d     = (double)s - (double)T_i                         (exact)
 *     S1    = sum d,  S2 = sum d * d                          (the product and every addition rounded once)
 *     mu64  = T_i + S1 / K
 *     var64 = max(S2 / K - (S1 / K)^2, 0)
 *   The sums of a row run per lane group g = (n mod 16) / 4 over its cohort rows in increasing n and merge as (g0 + g1) + (g2 +
 *   g3): an order the cohort alone fixes.  Samuelson's inequality, (mu - T)^2 <= (K - 1) var, bounds what the subtraction
 *   loses to about log2 K bits of float64.
 *
 * THE OUTPUTS, each (S) f32:
 *     thr[i] = T_i
 *     mu[i]  = (float)mu64
 *     sd[i]  = fmaxf((float)sqrt(var64), sd_floor)            (sd_floor > 0 is an argument)
 *     r[i]   = 1.0f / sd[i]                                   (correctly rounded)
 *   If any s(i, .) is not finite, the four outputs of row i are NaN and FHVAE_SN_NONFINITE is ORed into the status word; no
 *   other row changes a bit.  A row's four outputs are a function of that row and the cohort alone: bitwise the same alone, in
 *   any batch, at any position and through any leading dimension.  There are no floating-point atomics.
 *
 * THE NORMALISED SCORE of a pair, with s = (dot(i, j) + (a[i] + a[j])) + c as in include/fhvae_spk.h:
 *     sn(i, j) = 0.5f * ((s - mu[i]) * r[i] + (s - mu[j]) * r[j])        (every operation rounded once, no fused multiply-add)
 *   The outer addition commutes: sn(i, j) == sn(j, i) bit for bit.  sn does not change under s -> alpha s + beta (alpha > 0)
 *   applied to pair and cohort scores alike.  With mu = 0 and r = 1, sn == s exactly (s + s and the halving are exact).
 *
 *   fhvae_sn_range, fhvae_sn_hist and fhvae_sn_trials are fhvae_spk_llr_range, fhvae_spk_llr_hist and fhvae_spk_llr_trials
 *   with sn in place of s: the same trials (i < j, both labels >= 0, class 0 when the labels are equal), the same keys of the
 *   range and (+inf, -inf) for a class without a trial, the same bin expression, the same fmaf chain of a listed trial and the
 *   same index check.  A trial whose sn is NaN is in neither class and sets FHVAE_SN_NAN.
 *
 * Status: *status is an int32 device word the library only ORs bits into; the caller clears it.
 */
#ifndef FHVAE_SNORM_H
#define FHVAE_SNORM_H

#include "fhvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  FHVAE_SN_NAN = 1,       /* a trial's normalised score is NaN: it is counted in neither class */
  FHVAE_SN_BAD_INDEX = 2, /* a pair names a row outside [0, S): its score is NaN */
  FHVAE_SN_NONFINITE = 4  /* a cohort score of a row is not finite: the row's statistics are NaN */
};

#define FHVAE_SN_MAX_ROWS 16777216 /* S above 2^24: FHVAE_ERR_LIMIT */
#define FHVAE_SN_MAX_COHORT 1048576 /* Nc above 2^20: FHVAE_ERR_LIMIT */

/* bytes of workspace of fhvae_sn_range; 0 for arguments the calls below refuse.  Monotone in each argument. */
int64_t fhvae_sn_ws_bytes(int64_t S, int64_t D);

/* One launch, no workspace.  S or Nc < 1, a D, ld or ldz the all-pairs pass does not take, sd_floor not above 0 or not finite:
 * FHVAE_ERR_SHAPE; v or z off 16 bytes, anything else off 4: FHVAE_ERR_ALIGN; S above FHVAE_SN_MAX_ROWS or Nc above
 * FHVAE_SN_MAX_COHORT: FHVAE_ERR_LIMIT. */
int fhvae_sn_cohort_stats(const float* v, int64_t ld, const float* a, int64_t S, const float* z, int64_t ldz, const float* az, int64_t Nc,
                          int64_t D, float c, int64_t top, float sd_floor, float* mu, float* sd, float* r, float* thr, int32_t* status,
                          void* stream);

/* ws: fhvae_sn_ws_bytes(S, D) bytes, 4-byte aligned; nothing in it outlives the call.  mu and r (S) f32.  The rest as
 * fhvae_spk_llr_range. */
int fhvae_sn_range(const float* v, int64_t ld, const float* a, const float* mu, const float* r, const int32_t* label, int64_t S, int64_t D,
                   float c, void* ws, int64_t ws_bytes, float* range, int32_t* status, void* stream);

/* as fhvae_spk_llr_hist; hist is zeroed by the call */
int fhvae_sn_hist(const float* v, int64_t ld, const float* a, const float* mu, const float* r, const int32_t* label, int64_t S, int64_t D,
                  float c, float lo, float hi, int64_t n_bins, uint64_t* hist, int32_t* status, void* stream);

/* as fhvae_spk_llr_trials */
int fhvae_sn_trials(const float* v, int64_t ld, const float* a, const float* mu, const float* r, int64_t S, int64_t D, float c,
                    const int32_t* pairs, int64_t n, float* out, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
