/*
 * fhvae_falign.h -- forced alignment on per-frame scores (csrc/falign.hip): the best path of every utterance through the trellis
 * of its transcription, that path's score, and the first and last frame of every token.  It is the max-plus twin of the forward
 * sweep of include/fhvae_ctc.h plus a trace-back.  The entry points are exported from the same library as include/fhvae_hip.h and
 * follow its conventions (device pointers, enqueue only, FHVAE_ERR_* before any launch); they are declared here, not there, so
 * FHVAE_ABI_VERSION and the symbol set of that header are unchanged.
 *
 * The definition below is this project's; no other toolkit's binary was run against it.  tests/falign_ref.py is its scalar
 * float64 numpy oracle, and tests/test_falign_cpu.py compares that oracle with brute-force enumeration of all alignments.
 *
 * Every alignment of T frames takes exactly one score per frame, so the per-frame log-normaliser of a softmax is the same
 * constant for all paths: the best path of log-probabilities is the best path of the RAW scores, and the recursion below holds no
 * exp and no log.  Its float64 additions of f32 inputs are rounded once each and its maxima are exact, so an implementation is
 * pinned bit for bit.
 *
 * Inputs, all on the device:
 *   scores (n_frames, C) f32, leading dimension lds (a multiple of 4, at least C), 16-byte aligned
 *   utt_ptr (U + 1) int64: utterance u is the rows utt_ptr[u] .. utt_ptr[u + 1] - 1; monotone, utt_ptr[0] = 0, utt_ptr[U] =
 *     n_frames; an utterance may be empty and holds at most 2^31 - 1 frames
 *   labels int32 with lab_ptr (U + 1) int64, monotone from 0: the transcription of utterance u is labels[lab_ptr[u] ..
 *     lab_ptr[u + 1]); labels holds at least lab_ptr[U] entries (the library cannot check that)
 *   cell_ptr (U + 1) int64, monotone from 0: the back-pointers of utterance u live in the bytes ws + cell_ptr[u] ..
 *     ws + cell_ptr[u + 1]; it needs T_u S_u of them (S_u below), and cell_ptr[U] <= ws_bytes.  Their layout is private.
 *   2 <= C <= FHVAE_FA_MAX_CLASSES; blank in [0, C), or -1; a transcription holds at most FHVAE_FA_MAX_LABELS labels.
 *
 * Utterance u has rows z_0 .. z_{T-1} and labels l_1 .. l_L.  Two topologies:
 *   CTC, blank >= 0: the extended sequence l' of S = 2 L + 1 states, the blank at every even position (l'_{2 i - 1} = l_i).  A
 *     step stays, moves by one, or skips from s - 2 into s where l'_s != blank and l'_s != l'_{s-2} (the rule of fhvae_ctc.h).
 *     Start states {0, 1}; end states S - 1, then S - 2 (when L >= 1).
 *   HMM, blank == -1: S = L states, l'_s = l_{s+1}.  A step stays or moves by one.  Start state {0}, end state S - 1.
 *
 *     e_t(s)     = (double) z_t[l'_s]                                                  (exact)
 *     delta_0(s) = e_0(s) on the start states, -inf elsewhere
 *     for t >= 1 the candidates, in this order:  k = 0: delta_{t-1}(s)   k = 1: delta_{t-1}(s - 1)   k = 2: delta_{t-1}(s - 2)
 *       (k = 1 where s >= 1; k = 2 in CTC topology where the skip into s is allowed; a candidate that does not exist is -inf)
 *     b_t(s)     = the smallest k whose candidate is largest; 0 if every candidate is -inf
 *     delta_t(s) = candidate(b_t(s)) + e_t(s)                                          (float64, one rounding)
 *     end        : the end state of the larger delta_{T-1}; equal values go to S - 1
 *     score[u]   = that delta_{T-1}: the best path's sum of raw scores (not a log-probability)
 *     q_{T-1}    = the end state,   q_{t-1} = q_t - b_t(q_t)
 *
 * Outputs:
 *   state (n_frames) int32: state[utt_ptr[u] + t] = q_t
 *   seg (2 lab_ptr[U]) int32: seg[2 (lab_ptr[u] + i)] and the entry after it are the first and the last t at which the path sits
 *     in the state of label i (state 2 i + 1 in CTC topology, state i in HMM topology).  Every label of a feasible path has at
 *     least one frame.
 *   score (U) float64
 *
 *   L = 0 in CTC topology: every state is 0 and the score is the sum of z_t[blank] in increasing t.  T = 0 and L = 0: score 0.
 *   An utterance with no path of finite score, with T = 0 and L > 0, or (HMM topology) with L = 0 and T > 0 gets score -inf, its
 *   state and seg entries -1, and sets FHVAE_FA_INFEASIBLE.  A label outside [0, C), a label equal to a blank >= 0 or more than
 *   FHVAE_FA_MAX_LABELS labels gives the same outputs and sets FHVAE_FA_BAD_LABEL.  Both concern that utterance only.
 *   -inf scores are legal.  A NaN or +inf in an utterance's rows leaves that utterance's outputs unspecified but in range (state
 *   in [0, S) or -1, seg in [0, T) or -1) and changes no other utterance.
 *
 * DETERMINISM.  An utterance's outputs are a function of its rows and labels alone: bitwise the same alone, in any batch, at any
 * lds, at any position of the pointers, at any split of the workspace, and from run to run.
 *
 * Status: *status is an int32 device word the library only ORs bits into; the caller clears it.  A check kernel runs first:
 * pointer arrays that break their rules set FHVAE_FA_BAD_PTR, and with that bit set nothing is written.  Every index a kernel
 * forms is re-checked against n_frames, C, the pointers and ws_bytes, and a back-pointer read in the trace-back is clamped, so no
 * argument makes a kernel read or write outside its buffers (labels and seg beyond lab_ptr[U] excepted, see above).
 */
#ifndef FHVAE_FALIGN_H
#define FHVAE_FALIGN_H

#include "fhvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  FHVAE_FA_BAD_PTR = 1,   /* utt_ptr, lab_ptr or cell_ptr breaks its rules, or the back-pointers do not fit ws: nothing is written */
  FHVAE_FA_BAD_LABEL = 2, /* a label outside [0, C) or equal to a blank >= 0, or more than FHVAE_FA_MAX_LABELS labels */
  FHVAE_FA_INFEASIBLE = 4 /* the transcription has no path of finite score: score -inf, state and seg -1 */
};

#define FHVAE_FA_MAX_CLASSES 128 /* C above it: FHVAE_ERR_LIMIT */
#define FHVAE_FA_MAX_LABELS 256  /* labels of a transcription, at most: 513 trellis states in CTC topology */

/* bytes of back-pointers for `cells` = sum over the utterances of T_u S_u: one byte per cell, rounded up to 256; 0 for cells < 0
 * or beyond 2^59.  Monotone in cells. */
int64_t fhvae_fa_ws_bytes(int64_t cells);

/* state (n_frames) int32, seg (2 lab_ptr[U]) int32, score (U) float64.  C < 2, blank outside [-1, C), n_frames, U or ws_bytes
 * < 0, lds < C: FHVAE_ERR_SHAPE; lds no multiple of 4, scores or ws off 16 bytes, another pointer off its element:
 * FHVAE_ERR_ALIGN; C above FHVAE_FA_MAX_CLASSES, U above 2^31 - 1, n_frames above 2^52: FHVAE_ERR_LIMIT.  U == 0: returns 0,
 * launches nothing. */
int fhvae_fa_align(const float* scores, int64_t lds, int64_t n_frames, int64_t C, int64_t blank, const int64_t* utt_ptr,
                   const int32_t* labels, const int64_t* lab_ptr, const int64_t* cell_ptr, int64_t U, int32_t* state, int32_t* seg,
                   double* score, int32_t* status, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
