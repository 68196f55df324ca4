/*
 * fhvae_probe.h -- a linear probe (multinomial logistic regression) on frame-level rows (csrc/probe.hip): every row's
 * log-sum-exp, arg-max class and negative log-likelihood, their totals, and the gradient of the summed negative log-likelihood
 * with respect to the class table and the bias, with no (N, C) array of any kind.  The entry points are exported from the same
 * library as include/fhvae_hip.h and follow its conventions (device pointers, enqueue only, FHVAE_ERR_* before any launch); they
 * are declared here, not there, so FHVAE_ABI_VERSION and the symbol set of that header are unchanged.
 *
 * The definitions below are this project's: nothing here runs scikit-learn, and nothing was cross-checked against it.
 *
 * THE MODEL ON THE DEVICE.  W values per row, a multiple of 16 in [16, FHVAE_PROBE_MAX_W] (the widths of the all-pairs pass,
 * csrc/allpairs_f32.h; the Python layer zero-pads other widths).  Everything on the device:
 *   x    (N, W) f32, leading dimension ldx
 *   tab  (C, W) f32, leading dimension ldt: the class weights
 *   cst  (C) f32: the bias
 *   y    (N) int32: the class of a row; a value outside [0, C) means "unlabelled" (no index is ever formed from such a value)
 *   The leading dimensions are multiples of 4 and at least W, x and tab 16-byte aligned, the other pointers aligned to their
 *   element.  1 <= N <= FHVAE_PROBE_MAX_ROWS, 1 <= C <= FHVAE_PROBE_MAX_CLASSES.
 *
 * LOGITS, all in f32:
 *     dot(n, c) = x[n] . tab[c]      the dot of csrc/allpairs_f32.h over W columns, in its documented order: one fmaf chain of
 *                                    W terms from 0.  It does not depend on which of the two rows is the stationary one, so
 *     l(n, c)   = cst[c] + dot(n, c) (one rounding) has the SAME BITS in both passes below.
 *
 * PASS 1 (fhvae_probe_rows): the rows stationary, the classes streamed.
 *     lse[n]  = m + logf(s),  m = max_c l(n, c),  s = sum_c expf(l(n, c) - m)    in THE ORDER below
 *     pred[n] = the c of the largest l(n, c); equal values go to the smallest c
 *     nll[n]  = lse[n] - l(n, y[n]) (one rounding) for a labelled row, 0 for an unlabelled one
 *   THE ORDER (that of fhvae_gmm.h).  The classes are met in groups of four consecutive c, c = 4 j .. 4 j + 3 (c >= C: l = -inf).
 *   Group j belongs to lane a = j mod 4 of the row's four lanes; a lane meets its groups in increasing j and keeps (m, s, bc),
 *   from (-inf, 0, 0).  Per group, with its four values l_0 .. l_3:
 *     b = m;  for r = 0 .. 3:  if l_r > b:  b = l_r, bc = 4 j + r
 *     if b > m:        s = s * expf(m - b),  m = b
 *     for r = 0 .. 3:  if l_r != -inf:  s = s + expf(l_r - m)
 *   At the end, over the lanes a = 0 .. 3 in this order: M = max_a m_a;  S = sum_a (s_a == 0 ? 0 : s_a * expf(m_a - M)) from 0;
 *   lse = M + logf(S);  pred is the bc_a of the largest m_a, equal ones: the smallest bc_a.  expf and logf are the device
 *   library's, a few ulp each (the tests' bounds allow for them).
 *   A row's lse, pred and nll are a function of that row, tab, cst and its y alone: bitwise the same alone, in any batch and at
 *   any position of a workgroup's tile of 256 rows.  Bitwise equal (tab row, cst) pairs give bitwise equal l.  A row that holds
 *   a NaN gets lse NaN, pred 0 and (if labelled) nll NaN, and changes no other row; it does make totals[0] NaN.
 *   TOTALS, three float64: totals[0] = sum nll, totals[1] = the number of labelled rows, totals[2] = the number of labelled rows
 *   with pred == y.  The rows are cut into slices of FHVAE_PROBE_SLICE consecutive rows from row 0.  Within slice s, lane j
 *   (0 .. 63) adds (double)value of rows 1024 s + j + 64 k in increasing k from 0; the 64 lane sums are added pairwise over lane
 *   distances 32, 16, 8, 4, 2, 1 (a + b commutes: every lane ends with the same bits).  Then the slice sums are added in
 *   increasing s from 0.  No floating-point atomics.
 *
 * PASS 2 (fhvae_probe_grad): the classes stationary, the rows streamed; lse (N) f32 as pass 1 wrote it.
 *     r(n, c)  = expf(l(n, c) - lse[n]) - [c == y[n]]     for a labelled row (f32, one rounding each); 0 for an unlabelled row
 *     grad[c][d] = sum_n r(n, c) x[n][d]  (d < W)         grad[c][W] = sum_n r(n, c)
 *   grad is (C, W + 1) float64, dense.  r lives in registers only: no (N, C) array exists in the call or in its workspace.
 *   Within a slice of FHVAE_PROBE_SLICE rows each entry is ONE f32 fmaf chain from 0 over the slice's rows, sixteen rows at a time
 *   in increasing row, within sixteen rows b .. b + 15 in the order r = 0 .. 3 of v_mfma_f32_16x16x4_f32 instructions, each of
 *   which adds the rows b + r, b + 4 + r, b + 8 + r, b + 12 + r in the hardware's fixed order; it is stored as an f32 partial.
 *   Over the slices, in float64: grad = 0, then grad += (double)partial[slice] in increasing slice.  No floating-point
 *   atomics: the result depends on x, y, tab, cst, lse and N alone, not on the grid or on how many classes a wave holds.
 *   An unlabelled row enters with r = 0 AND x = 0 (selected, not multiplied): whatever its x holds, NaN included, changes nothing.
 *   A labelled row that holds a NaN (its lse is NaN) makes every entry of grad NaN.
 *   Bound per entry against the float64 sum of the float64 r: the error of r (see tests/probe_ref.py) times |x|, plus
 *   (FHVAE_PROBE_SLICE + 3) 2^-24 sum_n |r| |x|.
 *
 * Every index a kernel forms is re-checked against N, C and W, so no argument makes a kernel read or write outside its buffers.
 */
#ifndef FHVAE_PROBE_H
#define FHVAE_PROBE_H

#include "fhvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FHVAE_PROBE_SLICE 1024           /* rows per slice of the two-level sums */
#define FHVAE_PROBE_MAX_W 128            /* W a multiple of 16 in [16, 128] */
#define FHVAE_PROBE_MAX_ROWS 1073741824  /* N above 2^30: FHVAE_ERR_LIMIT */
#define FHVAE_PROBE_MAX_CLASSES 65536    /* C above 2^16: FHVAE_ERR_LIMIT */

/* bytes of workspace of either pass for N rows, C classes of W values: the f32 partials (slices, C, W + 1) and the float64
 * partials (slices, 3), each rounded up to 256 bytes; 0 for arguments the calls below refuse.  Monotone in N, C and W. */
int64_t fhvae_probe_ws_bytes(int64_t N, int64_t C, int64_t W);

/* lse (N) f32, pred (N) int32, nll (N) f32, totals (3) float64.  ws: fhvae_probe_ws_bytes(N, C, W) bytes, 16-byte aligned;
 * nothing in it outlives the call.  N, C < 1, a W outside the rule, a leading dimension below W, ws_bytes too small:
 * FHVAE_ERR_SHAPE; a pointer or leading dimension off its alignment: FHVAE_ERR_ALIGN; N, C above their limits: FHVAE_ERR_LIMIT. */
int fhvae_probe_rows(const float* x, int64_t ldx, int64_t N, int64_t W, const float* tab, int64_t ldt, const float* cst, int64_t C,
                     const int32_t* y, float* lse, int32_t* pred, float* nll, double* totals, void* ws, int64_t ws_bytes,
                     void* stream);

/* lse (N) f32 as fhvae_probe_rows wrote it; grad (C, W + 1) float64.  The argument errors of fhvae_probe_rows. */
int fhvae_probe_grad(const float* x, int64_t ldx, int64_t N, int64_t W, const float* tab, int64_t ldt, const float* cst, int64_t C,
                     const int32_t* y, const float* lse, double* grad, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
