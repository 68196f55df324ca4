/*
 * fhvae_gmm.h -- a diagonal-covariance Gaussian mixture on frame-level rows (csrc/gmm.hip): every row's log-likelihood and
 * arg-max component, its posteriors, and the sufficient statistics of an EM step.  The entry points are exported from the same
 * library as include/fhvae_hip.h and follow its conventions (device pointers, enqueue only, FHVAE_ERR_* before any launch);
 * they are declared here, not there, so FHVAE_ABI_VERSION and the symbol set of that header are unchanged.
 *
 * The definitions below are this project's: nothing here runs scikit-learn or Kaldi, and nothing was cross-checked against them.
 *
 * THE MODEL ON THE DEVICE.  D values per row, Dp = D rounded up to a multiple of 8, 8 <= Dp <= FHVAE_GMM_MAX_DP, W = 2 Dp (a
 * multiple of 16 in [16, 128]: the widths of the all-pairs pass, csrc/allpairs_f32.h).  Everything on the device:
 *   x    (N, Dp) f32, leading dimension ldx; columns [D, Dp) hold 0.
 *   tab  (K, W)  f32, leading dimension ldt: columns [0, Dp) hold p1[k][d] = mu[k][d] / var[k][d], columns [Dp, 2 Dp) hold
 *        p2[k][d] = -1 / (2 var[k][d]); the padding columns d >= D of either half hold 0.
 *   cst  (K) f32 = log w[k] - (D log 2pi + sum_d log var[k][d] + sum_d mu[k][d]^2 / var[k][d]) / 2, with the TRUE D, computed
 *        in float64 and rounded once.  A component of weight 0 has cst = -inf.
 *   The leading dimensions are multiples of 4 and at least the width, the pointers 16-byte aligned.  1 <= N <=
 *   FHVAE_GMM_MAX_ROWS, 1 <= K <= FHVAE_GMM_MAX_COMP.
 *
 * LOG-LIKELIHOOD (fhvae_gmm_loglik), all in f32:
 *     q[n][d]  = x[n][d] * x[n][d]                            one rounding
 *     dot(n,k) = [x[n], q[n]] . tab[k]                        the dot of csrc/allpairs_f32.h over W columns, in its documented
 *                                                             order: one fmaf chain of W terms from 0
 *     l(n, k)  = cst[k] + dot(n, k)                           one rounding
 *     loglik[n] = m + logf(s),  m = max_k l(n, k),  s = sum_k expf(l(n, k) - m)    in THE ORDER below
 *     label[n]  = the k of the largest l(n, k); equal values go to the smallest k
 *   THE ORDER.  The components are met in groups of four consecutive k, k = 4 j .. 4 j + 3 (k >= K: l = -inf).  Group j belongs
 *   to lane a = j mod 4 of the row's four lanes; a lane meets its groups in increasing j and keeps (m, s, bk), from
 *   (-inf, 0, 0).  Per group, with its four values l_0 .. l_3:
 *     b = m;  for r = 0 .. 3:  if l_r > b:  b = l_r, bk = 4 j + r
 *     if b > m:        s = s * expf(m - b),  m = b
 *     for r = 0 .. 3:  if l_r != -inf:  s = s + expf(l_r - m)
 *   At the end, over the lanes a = 0 .. 3 in this order: M = max_a m_a;  S = sum_a (s_a == 0 ? 0 : s_a * expf(m_a - M)) from 0;
 *   loglik = M + logf(S);  the label is the bk_a of the largest m_a, equal ones: the smallest bk_a.  expf and logf are the
 *   device library's, a few ulp each (the tests' bound allows for them).
 *   A row's outputs are a function of that row, tab and cst alone: bitwise the same alone, in any batch and at any position of a
 *   workgroup's tile of 256 rows.  Bitwise equal (tab row, cst) pairs give bitwise equal l.  A component with cst = -inf never
 *   wins and adds 0 to s (a model whose every cst is -inf is the caller's to refuse: loglik would be NaN).  A row that holds a
 *   NaN gets loglik NaN and label 0 and changes no other row.
 *
 * POSTERIORS (fhvae_gmm_post): the same pass again, l(n, k) by the same code in the same order, so with the same bits;
 *     post[n][k] = expf(l(n, k) - loglik[n])
 *   written to post (N, K) f32, leading dimension ldp (a multiple of 4, >= K, post 16-byte aligned) as 16-byte stores of a
 *   group of four k where the whole group lies below K.  Columns [K, ldp) are not touched.
 *
 * SUFFICIENT STATISTICS (fhvae_gmm_stats), from x and post:
 *     nk[k] = sum_n post[n][k]     sx[k][d] = sum_n post[n][k] x[n][d]     sxx[k][d] = sum_n post[n][k] q[n][d]
 *   with q as above (x squared in f32, one rounding).  The rows are cut into slices of FHVAE_GMM_SLICE consecutive rows from
 *   row 0 (the last one shorter).  Within a slice each entry is ONE f32 fmaf chain from 0 over the slice's rows in increasing
 *   row (v_mfma_f32_16x16x4_f32: four rows per instruction, added in the hardware's fixed order) and is written to the workspace
 *   as an f32 partial.  Over the slices, in float64: out = (accumulate ? out : 0), then out += (double)partial[slice] in
 *   increasing slice.  So a call with `accumulate` on the rows from a slice boundary on continues the sum of the call before
 *   it bit for bit.  No floating-point atomics: the result depends on x, post and N alone, not on the grid.
 *     nk (K) float64;  sx, sxx (K, Dp) float64, dense (leading dimension Dp); columns [D, Dp) come out 0.
 *   Bound per entry against the float64 sums of the same post: (FHVAE_GMM_SLICE + 3) 2^-24 sum_n post |a|.
 *
 * Every index a kernel forms is re-checked against N, K and Dp, so no argument makes a kernel read or write outside its buffers.
 */
#ifndef FHVAE_GMM_H
#define FHVAE_GMM_H

#include "fhvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FHVAE_GMM_SLICE 1024           /* rows per slice of the statistics' two-level sum */
#define FHVAE_GMM_MAX_DP 64            /* Dp a multiple of 8 in [8, 64] */
#define FHVAE_GMM_MAX_ROWS 1073741824  /* N above 2^30: FHVAE_ERR_LIMIT */
#define FHVAE_GMM_MAX_COMP 1048576     /* K above 2^20: FHVAE_ERR_LIMIT */

/* bytes of workspace of fhvae_gmm_stats for N rows, K components of Dp values; 0 for arguments the calls below refuse.
 * Monotone in N and in K. */
int64_t fhvae_gmm_ws_bytes(int64_t N, int64_t K, int64_t Dp);

/* loglik (N) f32, label (N) int32 or NULL.  N, K < 1, a Dp outside the rule, a leading dimension below its width:
 * FHVAE_ERR_SHAPE; a pointer or leading dimension off its alignment: FHVAE_ERR_ALIGN; N, K above their limits:
 * FHVAE_ERR_LIMIT. */
int fhvae_gmm_loglik(const float* x, int64_t ldx, int64_t N, int64_t Dp, const float* tab, int64_t ldt, const float* cst, int64_t K,
                     float* loglik, int32_t* label, void* stream);

/* loglik (N) f32 as fhvae_gmm_loglik wrote it; post (N, K) f32 with ldp.  The argument errors of fhvae_gmm_loglik. */
int fhvae_gmm_post(const float* x, int64_t ldx, int64_t N, int64_t Dp, const float* tab, int64_t ldt, const float* cst, int64_t K,
                   const float* loglik, float* post, int64_t ldp, void* stream);

/* ws: fhvae_gmm_ws_bytes(N, K, Dp) bytes, 16-byte aligned; nothing in it outlives the call.  accumulate != 0 adds onto what
 * nk, sx, sxx hold.  The argument errors of fhvae_gmm_loglik; ws_bytes below fhvae_gmm_ws_bytes(N, K, Dp): FHVAE_ERR_SHAPE. */
int fhvae_gmm_stats(const float* x, int64_t ldx, int64_t N, int64_t Dp, const float* post, int64_t ldp, int64_t K, void* ws,
                    int64_t ws_bytes, double* nk, double* sx, double* sxx, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif
