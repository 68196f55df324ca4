/*
 * fhvae_viterbi.h -- phone recognition on per-frame scores (csrc/viterbi.hip): a batched Viterbi decoder (the best state
 * sequence of every utterance under a dense transition table) and a batched Levenshtein aligner (substitutions, deletions,
 * insertions and correct tokens of every (reference, hypothesis) pair).  The entry points are exported from the same library as
 * include/fhvae_hip.h and follow its conventions (device pointers, enqueue only, FHVAE_ERR_* before any launch); they are
 * declared here, not there, so FHVAE_ABI_VERSION and the symbol set of that header are unchanged.
 *
 * The definitions below are this project's: no Kaldi, HTK or sclite binary exists here to compare with, and nothing was
 * cross-checked against one.  Both are dynamic programmes over integers or over f32 additions rounded once and f32 maxima (which
 * are exact), so the results are pinned bit for bit by scalar oracles (tests/viterbi_ref.py); there is no tolerance.
 *
 * VITERBI.  Everything on the device:
 *   emit  (n_frames, C) f32, leading dimension lde (a multiple of 4, at least C), 16-byte aligned: the score of state c at a frame
 *   trans (C, C) f32, dense: trans[p][c] is the score of going from state p to state c
 *   init  (C) f32; fin (C) f32 or NULL
 *   utt_ptr (U + 1) int64: utterance u is the rows utt_ptr[u] .. utt_ptr[u + 1] - 1 of emit.  The rules of fhvae_qbe.h:
 *     monotone, utt_ptr[0] = 0, utt_ptr[U] = n_frames; an utterance may be empty and holds at most 2^31 - 1 frames.
 *   1 <= C <= FHVAE_VIT_MAX_STATES.  -inf is a legal value anywhere (a forbidden transition, a left-to-right topology).  NaN and
 *   +inf are outside the contract (see MISUSE).
 *
 * Recursion for an utterance of m >= 1 frames with rows e_0 .. e_{m-1}; f32, one rounding per addition:
 *     d_0[c] = init[c] + e_0[c]
 *     t >= 1:  v(p) = d_{t-1}[p] + trans[p][c]      b_t[c] = the SMALLEST p whose v(p) is largest
 *              d_t[c] = v(b_t[c]) + e_t[c]
 *     end:     w[c] = d_{m-1}[c]   (with fin: w[c] = d_{m-1}[c] + fin[c], one rounding)
 *              q_{m-1} = the smallest c whose w[c] is largest;  score = w[q_{m-1}];  q_{t-1} = b_t[q_t];  path = q
 *   The maximum of f32 values is exact, so the result does not depend on the order of a reduction; only the tie rule is carried,
 *   as a (value, index) pair compared lexicographically.  All candidates -inf is a tie: index 0 wins, and the score is -inf.
 *   An empty utterance gets score -inf and no path entry.
 *   NO RENORMALISATION per step: the magnitude of d grows with m (about m times the typical frame score), and the resolution of
 *   every comparison is one f32 ulp of the running score: at |d| near 2^20 (a 10-minute utterance at 10 nats per frame) two
 *   paths closer than 2^-3 are a tie and go to the smaller index.  That is part of the definition, and the oracle has it too.
 *   An utterance's path and score are a function of its rows, trans, init and fin alone: bitwise the same alone, in any batch, at
 *   any lde and at any position of utt_ptr.
 *   MISUSE: an utterance whose emissions hold a NaN gets unspecified path values that lie in [0, C) and an unspecified score.  It
 *   changes no other utterance.
 *
 * Outputs: path (n_frames) int32, score (U) f32.  ws: fhvae_vit_ws_bytes(n_frames, C) bytes of back-pointers, one byte per
 * (frame, state); nothing in it outlives the call.
 *
 * LEVENSHTEIN.  ref and hyp are int32 token arrays with int64 CSR pointers ref_ptr, hyp_ptr (U + 1 each, monotone from 0); pair
 * u is ref[ref_ptr[u] .. ref_ptr[u + 1]) against hyp[hyp_ptr[u] .. hyp_ptr[u + 1]).  Tokens are compared for equality only: any
 * int32 value is a token.  Over a ref prefix of i tokens and a hyp prefix of j tokens each cell carries (cost, S, D, I, Cor):
 *     [0][j] = (j, 0, 0, j, 0): j insertions          [i][0] = (i, 0, i, 0, 0): i deletions
 *     elsewhere the candidates are, IN THIS ORDER:
 *       diagonal [i-1][j-1]: cost + [ref_i != hyp_j]; counts one S (unequal) or one Cor (equal)
 *       up       [i-1][j]:   cost + 1; counts one D
 *       left     [i][j-1]:   cost + 1; counts one I
 *     the smallest cost wins, a tie goes to the EARLIER candidate in that order; the cell's counts are the winner's plus its own one.
 *   counts (U, 4) int32 = (S, D, I, Cor) of cell [|ref|][|hyp|].  S + D + Cor = |ref|, S + I + Cor = |hyp|, S + D + I = cost.
 *   A ref of more than FHVAE_EDIT_MAX_REF tokens sets FHVAE_EDIT_BAD_REF and gets -1 four times, for that pair only.  A hyp has any
 *   length up to 2^31 - 1 and is streamed.  A pair's counts are a function of that pair alone.
 *
 * Status: *status is an int32 device word the library only ORs bits into; the caller clears it.  A check kernel runs first:
 * pointers that break their rules set FHVAE_VIT_BAD_PTR / FHVAE_EDIT_BAD_PTR, and with that bit set the kernel behind it writes
 * nothing.  Every index a kernel forms is re-checked against n_frames, C and the pointers, and a back-pointer read in the
 * trace-back is clamped to [0, C), so no argument makes a kernel read or write outside its buffers.
 */
#ifndef FHVAE_VITERBI_H
#define FHVAE_VITERBI_H

#include "fhvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  FHVAE_VIT_BAD_PTR = 1 /* utt_ptr is not monotone, does not run from 0 to n_frames, or an utterance is too long */
};
enum {
  FHVAE_EDIT_BAD_PTR = 1, /* ref_ptr or hyp_ptr is not monotone from 0, or a hyp is longer than 2^31 - 1 */
  FHVAE_EDIT_BAD_REF = 2  /* a ref is longer than FHVAE_EDIT_MAX_REF: that pair's counts are -1 */
};

#define FHVAE_VIT_MAX_STATES 128 /* C above it: FHVAE_ERR_LIMIT */
#define FHVAE_EDIT_MAX_REF 256   /* tokens of a ref, at most */

/* bytes of back-pointers fhvae_vit_decode needs: n_frames * C rounded up to 256; 0 for arguments the call refuses (n_frames < 0,
 * C outside [1, FHVAE_VIT_MAX_STATES]).  Monotone in n_frames and C. */
int64_t fhvae_vit_ws_bytes(int64_t n_frames, int64_t C);

/* path (n_frames) int32, score (U) f32.  C < 1, n_frames or U < 0, lde < C, ws_bytes below fhvae_vit_ws_bytes(n_frames, C):
 * FHVAE_ERR_SHAPE; lde no multiple of 4, emit off 16 bytes, another pointer off its element: FHVAE_ERR_ALIGN; C above
 * FHVAE_VIT_MAX_STATES, U above 2^31 - 1: FHVAE_ERR_LIMIT.  fin may be NULL.  U == 0: returns 0, launches nothing. */
int fhvae_vit_decode(const float* emit, int64_t lde, int64_t n_frames, int64_t C, const float* trans, const float* init,
                     const float* fin, const int64_t* utt_ptr, int64_t U, int32_t* path, float* score, int32_t* status, void* ws,
                     int64_t ws_bytes, void* stream);

/* counts (U, 4) int32.  U < 0: FHVAE_ERR_SHAPE; U above 2^31 - 1: FHVAE_ERR_LIMIT; a pointer off its element: FHVAE_ERR_ALIGN.
 * U == 0: returns 0, launches nothing. */
int fhvae_edit_align(const int32_t* ref, const int64_t* ref_ptr, const int32_t* hyp, const int64_t* hyp_ptr, int64_t U,
                     int32_t* counts, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
