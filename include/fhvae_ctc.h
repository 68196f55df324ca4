/*
 * fhvae_ctc.h -- connectionist temporal classification on per-frame logits (csrc/ctc.hip): the negative log-likelihood of every
 * utterance's transcription summed over all its alignments, and its gradient with respect to the logits, by one forward-backward
 * pass per utterance.  The entry points are exported from the same library as include/fhvae_hip.h and follow its conventions
 * (device pointers, enqueue only, FHVAE_ERR_* before any launch); they are declared here, not there, so FHVAE_ABI_VERSION and
 * the symbol set of that header are unchanged.
 *
 * The definition below is this project's.  It is the usual CTC of Graves et al. (2006) in the log domain; no other toolkit's
 * binary was run against it.  tests/ctc_ref.py is its float64 numpy oracle, and tests/test_ctc_cpu.py compares that oracle
 * with torch.nn.functional.ctc_loss, with brute-force enumeration and with finite differences.
 *
 * Inputs, all on the device:
 *   logits (n_frames, C) f32, leading dimension ldz (a multiple of 4, at least C), 16-byte aligned
 *   utt_ptr (U + 1) int64: utterance u is the rows utt_ptr[u] .. utt_ptr[u + 1] - 1; monotone, utt_ptr[0] = 0, utt_ptr[U] =
 *     n_frames; an utterance may be empty and holds at most 2^31 - 1 frames
 *   labels int32 with lab_ptr (U + 1) int64, monotone from 0: the transcription of utterance u is labels[lab_ptr[u] ..
 *     lab_ptr[u + 1]); labels holds at least lab_ptr[U] entries (the library cannot check that)
 *   cell_ptr (U + 1) int64, monotone from 0: the float64 alpha rows of utterance u live at ws + 8 cell_ptr[u]; it needs
 *     T_u (2 L_u + 1) cells, and 8 cell_ptr[U] <= ws_bytes.  Only read when grad is given.
 *   2 <= C <= FHVAE_CTC_MAX_CLASSES, the blank included; 0 <= blank < C; a transcription holds at most FHVAE_CTC_MAX_LABELS labels.
 *
 * Utterance u has rows z_0 .. z_{T-1}, labels l_1 .. l_L and the extended sequence l' of S = 2 L + 1 entries, the blank at every
 * even position (l'_{2 i - 1} = l_i).  Everything is float64 on the device, from the f32 logits; lse(x ...) = m + log(sum
 * exp(x - m)) with m the largest x, and -inf if every x is -inf (never NaN):
 *     lp_t[c]    = (z_t[c] - m_t) - log sum_c exp(z_t[c] - m_t),  m_t the row maximum
 *     alpha_0(0) = lp_0[blank],  alpha_0(1) = lp_0[l_1],  every other state -inf
 *     alpha_t(s) = lse(alpha_{t-1}(s), alpha_{t-1}(s-1), [l'_s != blank and l'_s != l'_{s-2}] alpha_{t-1}(s-2)) + lp_t[l'_s]
 *     ll         = lse(alpha_{T-1}(S-1), alpha_{T-1}(S-2))          nll[u] = -ll
 *     beta_{T-1}(S-1) = beta_{T-1}(S-2) = 0,  every other state -inf
 *     beta_t(s)  = lse over s' in {s, s+1, s+2 where the skip into s+2 is allowed} of beta_{t+1}(s') + lp_{t+1}[l'_{s'}]
 *     occ_t[c]   = sum over the s with l'_s = c, in increasing s, of exp(alpha_t(s) + beta_t(s) - ll)
 *     grad[t][c] = (float)(exp(lp_t[c]) - occ_t[c])      the derivative of nll[u] with respect to z_t[c], rounded once
 *   -inf logits are legal: a class with bias -inf has probability 0.  L = 0 is legal: nll is the sum of -lp_t[blank].  An empty
 *   utterance with L = 0 has nll 0.
 *   An utterance whose transcription has no alignment (T < L + the number of equal neighbours, T = 0 with L > 0, a needed class at
 *   probability 0) gets nll = +inf and zero gradient rows and sets FHVAE_CTC_INFEASIBLE.  A label outside [0, C), a label equal
 *   to blank or L above the limit gives the same outputs and sets FHVAE_CTC_BAD_LABEL.  Both concern that utterance only.
 *   A NaN (or a row of -inf only, or +inf) in an utterance's logits leaves that utterance's outputs unspecified and changes no
 *   other utterance.
 *
 * DETERMINISM.  An utterance's nll and gradient rows are a function of its rows and labels alone: bitwise the same alone, in any
 * batch, at any ldz / ldg, at any position of the pointers, with or without grad (nll), and from run to run.  There is no
 * floating-point atomic; every sum has a fixed order.
 *
 * Outputs: nll (U) float64; grad (n_frames, C) f32 with leading dimension ldg (a multiple of 4, at least C, 16-byte aligned), or
 * NULL: then only nll is computed and ws and cell_ptr may be NULL.  Columns c >= C of grad are never written.
 *
 * Status: *status is an int32 device word the library only ORs bits into; the caller clears it.  A check kernel runs first:
 * pointer arrays that break their rules set FHVAE_CTC_BAD_PTR, and with that bit set nothing is written.  Every index a kernel
 * forms is re-checked against n_frames, C, the pointers and ws_bytes, so no argument makes a kernel read or write outside its
 * buffers (labels beyond lab_ptr[U] excepted, see above).
 */
#ifndef FHVAE_CTC_H
#define FHVAE_CTC_H

#include "fhvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  FHVAE_CTC_BAD_PTR = 1,   /* utt_ptr, lab_ptr or cell_ptr breaks its rules, or the alpha rows do not fit ws: nothing is written */
  FHVAE_CTC_BAD_LABEL = 2, /* a label outside [0, C) or equal to blank, or more than FHVAE_CTC_MAX_LABELS labels: nll = +inf */
  FHVAE_CTC_INFEASIBLE = 4 /* the transcription has no alignment of probability above 0: nll = +inf, zero gradient rows */
};

#define FHVAE_CTC_MAX_CLASSES 128 /* C above it: FHVAE_ERR_LIMIT */
#define FHVAE_CTC_MAX_LABELS 256  /* labels of a transcription, at most: 513 trellis states */

/* bytes of float64 alpha rows for `cells` = sum over the utterances of T_u (2 L_u + 1), rounded up to 256; 0 for cells < 0 or
 * beyond 2^59.  Monotone in cells. */
int64_t fhvae_ctc_ws_bytes(int64_t cells);

/* nll (U) float64, grad (n_frames, C) f32 or NULL.  C < 2, blank outside [0, C), n_frames, U or ws_bytes < 0, ldz < C, ldg < C:
 * FHVAE_ERR_SHAPE; ldz or ldg no multiple of 4, logits, grad or ws off 16 bytes, another pointer off its element:
 * FHVAE_ERR_ALIGN; C above FHVAE_CTC_MAX_CLASSES, U above 2^31 - 1, n_frames above 2^52: FHVAE_ERR_LIMIT.  With grad NULL, ldg,
 * cell_ptr, ws and ws_bytes are ignored.  U == 0: returns 0, launches nothing. */
int fhvae_ctc_loss(const float* logits, int64_t ldz, int64_t n_frames, int64_t C, int64_t blank, const int64_t* utt_ptr,
                   const int32_t* labels, const int64_t* lab_ptr, const int64_t* cell_ptr, int64_t U, double* nll, float* grad,
                   int64_t ldg, int32_t* status, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
