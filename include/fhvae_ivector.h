/*
 * fhvae_ivector.h -- i-vector extraction (csrc/ivector.hip): the Baum-Welch statistics of every utterance of a batch in one
 * launch, and the batched float64 factor / solve / inverse of the utterances' posterior precisions.  The entry points are
 * exported from the same library as include/fhvae_hip.h and follow its conventions (device pointers, enqueue only, FHVAE_ERR_*
 * before any launch); they are declared here, not there, so FHVAE_ABI_VERSION and the symbol set of that header are unchanged.
 *
 * The definitions below are this project's; no Kaldi binary (ivector-extract) was available to compare with.
 *
 * THE MODEL (ivector.py holds the host side, in float64).  A UBM of gmm.py with C components of D values, Dp = D rounded up to
 * a multiple of 8 (Dp <= 64), means m_c and variances s_c^2.  For utterance u with rows [ptr[u], ptr[u + 1]) and posteriors
 * g_t(c) (gmm.posteriors, not pruned):
 *     n_c(u) = sum_t g_t(c)                 f_c(u) = sum_t g_t(c) x_t                          (fhvae_iv_stats)
 *     ft_c(u) = (f_c(u) - n_c(u) m_c) / s_c     a row of C Dp values, padding columns 0          (host, float64)
 *   The extractor Tt is (C Dp, R), 1 <= R <= FHVAE_IV_MAX_RANK, Tt_c its (Dp, R) block, M_c = Tt_c^T Tt_c:
 *     L_u = I + sum_c n_c(u) M_c     b_u = Tt^T ft(u)     w_u = L_u^-1 b_u     E_u = L_u^-1 + w_u w_u^T     (fhvae_iv_solve)
 *     Q = sum_u [ -1/2 log det L_u + 1/2 b_u^T w_u ]      the part of the marginal log-likelihood that depends on Tt
 *   EM: A_c = sum_u n_c(u) E_u, K_c = sum_u ft_c(u) w_u^T, Tt_c <- K_c A_c^-1; minimum divergence: a second E-step with the new
 *   Tt, P = (1 / U) sum_u E_u = G G^T (Cholesky), Tt <- Tt G.  The UBM's variances are not re-estimated.
 *
 * STATISTICS (fhvae_iv_stats).  x (N, Dp) f32 with ldx, post (N, C) f32 with ldp, under the rules of include/fhvae_gmm.h (leading
 * dimensions multiples of 4 and at least the width, 16-byte aligned pointers, Dp a multiple of 8 in [8, 64]); utt_ptr (U + 1)
 * int64 ON THE DEVICE.  Utterance u is GOOD when 0 <= utt_ptr[u] <= utt_ptr[u + 1] <= N.  The arithmetic is fhvae_gmm_stats',
 * restricted to an utterance:
 *   The rows of a good utterance are cut into slices of FHVAE_IV_SLICE consecutive rows FROM ITS OWN FIRST ROW (the last one
 *   shorter).  Within a slice each entry of n and f is ONE f32 chain from 0 over the slice's rows in increasing row
 *   (v_mfma_f32_16x16x4_f32: four rows per instruction, added in the hardware's fixed order; n is the chain of g_t(c) * 1) and is
 *   written to the workspace as an f32 partial.  Over the slices, in float64: v = 0, then v += (double)partial[slice] in
 *   increasing slice; the output is (float)v, rounded once.  No floating-point atomics.
 *   So an utterance's n and f are a function of its own rows alone: bitwise the same alone, in any batch and at any position.
 *   n (U, C) f32 and f (U, C, Dp) f32 are dense; the padding columns [D, Dp) of f come out 0 (x holds 0 there).  An empty
 *   utterance gives zeros.  An utterance that is not good gives zeros and sets FHVAE_IV_BAD_PTR; nothing is read through its
 *   pointers.  (The workspace holds N / FHVAE_IV_SLICE + U slices, which pointers that are monotone as a whole never exceed; where
 *   good utterances overlap so that their slices do, those met later in u are zeroed with FHVAE_IV_BAD_PTR as well.)
 *   Bound per entry against the float64 sums of the same post: (FHVAE_IV_SLICE + 3) 2^-24 sum_t g |x| + 2^-24 |total|.
 *
 * SOLVE (fhvae_iv_solve), all in float64, one utterance at a time.  Lp (U, P) holds the lower triangle of the symmetric L_u packed
 * by rows, p = i (i + 1) / 2 + j for j <= i, P = R (R + 1) / 2; b (U, R).  fma(a, b, c) is the fused operation; every other
 * operation is rounded once; division is correctly rounded.  In this order:
 *   1. The root-free Cholesky factor L = G D G^T (G unit lower triangular, D = diag(d)), column j = 0 .. R - 1:
 *        u_k  = G[j][k] * d_k                                                                               (k < j)
 *        a_ij = the chain acc = fma(-G[i][k], u_k, acc) over k = 0 .. j - 1 from acc = L[i][j]              (i >= j)
 *        d_j = a_jj;   G[i][j] = a_ij / d_j                                                                 (i > j)
 *      No square root is taken.  A pivot d_j that is not positive or not finite sets FHVAE_IV_NOT_PD: that utterance's w, E and
 *      logdet are NaN, and no other utterance changes.
 *   2. z = G^-1 b by columns j = 0 .. R - 1:  z_i = fma(-G[i][j], z_j, z_i) for i > j    (z starts as b)
 *      y_j = z_j / d_j
 *      w = G^-T y by rows k = R - 1 .. 1:     y_j = fma(-G[k][j], y_k, y_j) for j < k;  w is what y then holds
 *   3. logdet = the chain s = s + log(d_j) over j = 0 .. R - 1 from 0 (log: the device library's)
 *   4. If E is asked for: H = G^-1 (unit lower triangular) by rows i = 0 .. R - 1:  for j < i, H[i][j] = -acc with
 *      acc = fma(G[i][k], H[k][j], acc) over k = j + 1 .. i - 1 from acc = G[i][j];  r_k = 1 / d_k.  Then for j <= i:
 *        E[i][j] = fma(w_i, w_j, s),  s the chain s = fma(H[k][i] * r_k, H[k][j], s) over k = i + 1 .. R - 1 from
 *                                   s = r_i (j = i) or r_i * H[i][j] (j < i), the product H[k][i] * r_k rounded once
 *      written packed like Lp.
 *   w does not depend on whether E or logdet is asked for.  An utterance's outputs are a function of its own Lp, b and R alone:
 *   one thread owns each chain, nothing is reduced across lanes, so they are bitwise the same alone and in any batch.
 *
 * Status: *status is an int32 device word the library only ORs bits into; the caller clears it.
 * Every index a kernel forms is re-checked against N, C, Dp, U and R, so no argument makes a kernel read or write outside its buffers.
 */
#ifndef FHVAE_IVECTOR_H
#define FHVAE_IVECTOR_H

#include "fhvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  FHVAE_IV_BAD_PTR = 1, /* an utterance's pointers decrease or leave [0, N]: its statistics are zeros */
  FHVAE_IV_NOT_PD = 2   /* a pivot is not positive or not finite: that utterance's w, E, logdet are NaN */
};

#define FHVAE_IV_SLICE 1024          /* rows per slice of the statistics' two-level sum, from the utterance's first row */
#define FHVAE_IV_MAX_RANK 128        /* R above it: FHVAE_ERR_LIMIT */
#define FHVAE_IV_MAX_UTT 4194304     /* U above 2^22: FHVAE_ERR_LIMIT */
#define FHVAE_IV_MAX_ROWS 1073741824 /* N above 2^30: FHVAE_ERR_LIMIT (FHVAE_GMM_MAX_ROWS) */
#define FHVAE_IV_MAX_COMP 1048576    /* C above 2^20: FHVAE_ERR_LIMIT (FHVAE_GMM_MAX_COMP) */

/* bytes of workspace of fhvae_iv_stats: the (U + 1) int64 slice offsets and the f32 partials (N / SLICE + U slices, C, Dp + 1);
 * 0 for arguments the call refuses.  Monotone in each argument. */
int64_t fhvae_iv_ws_bytes(int64_t N, int64_t U, int64_t C, int64_t Dp);

/* n (U, C) f32, f (U, C, Dp) f32, both dense.  ws: fhvae_iv_ws_bytes(N, U, C, Dp) bytes, 16-byte aligned; nothing in it outlives the
 * call.  N, U, C < 1, a Dp outside the rule, a leading dimension below its width, ws_bytes too small: FHVAE_ERR_SHAPE; x, post or ws
 * off 16 bytes, a leading dimension no multiple of 4, utt_ptr off 8 bytes, n, f or status off 4 bytes: FHVAE_ERR_ALIGN; N, U, C
 * above their limits: FHVAE_ERR_LIMIT. */
int fhvae_iv_stats(const float* x, int64_t ldx, int64_t N, int64_t Dp, const float* post, int64_t ldp, int64_t C, const int64_t* utt_ptr,
                   int64_t U, void* ws, int64_t ws_bytes, float* n, float* f, int32_t* status, void* stream);

/* Lp (U, P), b (U, R), w (U, R), E (U, P) or NULL, logdet (U) or NULL; all float64, dense.  No workspace.  U, R < 1:
 * FHVAE_ERR_SHAPE; a float64 pointer off 8 bytes, status off 4 bytes: FHVAE_ERR_ALIGN; R above FHVAE_IV_MAX_RANK or U above
 * FHVAE_IV_MAX_UTT: FHVAE_ERR_LIMIT. */
int fhvae_iv_solve(const double* Lp, const double* b, int64_t U, int64_t R, double* w, double* E, double* logdet, int32_t* status,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
