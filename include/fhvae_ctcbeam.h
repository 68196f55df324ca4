/*
 * fhvae_ctcbeam.h -- CTC prefix beam search on per-frame logits, with an optional label bigram (csrc/ctcbeam.hip): for every
 * utterance the labelling whose alignments together (not its single best path) score highest among the prefixes a beam of W
 * keeps, its length and its score.  The entry points are exported from the same library as include/fhvae_hip.h and follow its
 * conventions (device pointers, enqueue only, FHVAE_ERR_* before any launch); they are declared here, not there, so
 * FHVAE_ABI_VERSION and the symbol set of that header are unchanged.
 *
 * The definition below is this project's: the prefix search of Graves (2012) / Hannun et al. (2014) in the log domain with every
 * choice written out.  No other toolkit's binary was run against it.  tests/ctcbeam_ref.py is its float64 numpy oracle, written
 * from this text, and tests/test_ctcbeam_cpu.py compares that oracle with brute-force enumeration of all paths.
 *
 * Inputs, all on the device:
 *   logits (n_frames, C) f32, leading dimension ldz (a multiple of 4, at least C), 16-byte aligned
 *   utt_ptr (U + 1) int64: utterance u is the rows utt_ptr[u] .. utt_ptr[u + 1] - 1; monotone, utt_ptr[0] = 0, utt_ptr[U] =
 *     n_frames; an utterance may be empty and holds at most 2^31 - 1 frames
 *   2 <= C <= FHVAE_CB_MAX_CLASSES, the blank included; 0 <= blank < C
 *   the beam width 1 <= W <= FHVAE_CB_MAX_BEAM
 *   class_beam >= 0, a double; +inf: no class pruning
 *   lm: a (C + 1, C + 1) float64 table, dense, or NULL.  Row r is the previous label, row C the sentence start; column c is the
 *     next label, column C the sentence end.  The caller has scaled it and added any per-label bonus to the columns c < C: the
 *     kernel only ADDS entries.  -inf entries are legal and forbid a transition; +inf and NaN are not legal.  The blank's row
 *     and column are never read.  NULL: every entry is 0.
 *
 * Everything is float64 on the device.  lp_t and lse are exactly those of include/fhvae_ctc.h:
 *     lp_t[c] = (z_t[c] - m_t) - log sum_c exp(z_t[c] - m_t),  m_t the row maximum
 *     lse(a, b) = m + log(exp(a - m) + exp(b - m)),  m = max(a, b), and -inf if both are -inf (never NaN)
 *
 * A beam is an ordered list of at most W entries.  An entry is a label prefix -- no two entries hold the same labels -- with
 *     pb, pnb  the log mass of the prefix's alignments that end in the blank / in its last label
 *     lm       the table entries summed along the prefix, in label order, from 0
 *     last     its last label, or C for the empty prefix
 * Start: one entry, the empty prefix, pb = 0, pnb = -inf, lm = 0.  At frame t, with n entries in the beam:
 *     tot_i     = lse(pb_i, pnb_i)
 *     ext(i, c) = (c == last_i ? pb_i : tot_i) + lp_t[c]
 *     class c is OPEN when lp_t[c] >= max_c' lp_t[c'] - class_beam      (the maximum over all classes, the blank included)
 *   The candidates:
 *     stay(i), index i:
 *         pb'  = tot_i + lp_t[blank]
 *         pnb' = pnb_i + lp_t[last_i], or -inf for the empty prefix;
 *                if a beam entry j holds the prefix of i without its last label and last_i is open:
 *                pnb' = lse(pnb', ext(j, last_i))
 *         lm'  = lm_i
 *         score = lse(pb', pnb') + lm'
 *     extend(i, c), index W + i C + c, for every open c that is not the blank and for which no beam entry holds prefix_i + c:
 *         pb'  = -inf,   pnb' = ext(i, c),   lm' = lm_i + table[last_i][c]
 *         score = pnb' + lm'                                            (lse(-inf, x) is x exactly)
 *   A candidate with score -inf is never kept.  The new beam is the W best candidates by score, in decreasing score; equal
 *   scores (as numbers: -0 equals +0) go by candidate index, smaller first.
 *   After the last frame an entry's final score is (tot_i + lm_i) + table[last_i][C].  The result is the entry with the largest
 *   final score, the first such position of the beam (if every final score is -inf: position 0).  Outputs: its labels, their
 *   count, that score.  T = 0 gives the empty hypothesis with score (0 + 0) + table[C][C].
 *   A beam may empty out (no candidate above -inf at some frame): that utterance gets length 0 and score -inf and sets
 *   FHVAE_CB_EMPTY.  It concerns that utterance only.
 *
 * PREFIX IDENTITY IS BY LABEL SEQUENCE.  A prefix that fell out of the beam while one of its children stayed can be created
 * again by its parent; it is then the same prefix: its child merges into it (the stay rule) and it does not extend into that
 * child (the extend rule).  The kernel keeps one node per prefix in a per-utterance trie in the workspace, (parent node, label)
 * -> node, looked up for every kept extension before a node is made; node numbers follow the new beam's order, not thread timing.
 *
 * A NaN (or +inf, or a row of -inf only) in an utterance's logits leaves that utterance's outputs unspecified and changes no
 * other utterance.
 *
 * DETERMINISM.  An utterance's three outputs are a function of its rows, W, class_beam and the table alone: bitwise the same
 * alone, in any batch, at any ldz, at any position of the pointers and the workspace, and from run to run.  There is no
 * floating-point atomic; every sum has a fixed order.
 *
 * Outputs: hyp int32 of capacity n_frames: the labels of utterance u are hyp[utt_ptr[u] .. utt_ptr[u] + hyp_len[u]) (a
 * hypothesis never has more labels than frames; the rest of hyp is not written); hyp_len (U) int32; score (U) float64.
 *
 * Workspace: FHVAE_CB_NODE_BYTES per trie node, at most W new nodes a frame: utterance u's nodes start at byte
 * FHVAE_CB_NODE_BYTES * W * utt_ptr[u] of ws, so no pointer array is needed.  Its contents before the call do not matter.
 *
 * Status: *status is an int32 device word the library only ORs bits into; the caller clears it.  A check kernel runs first:
 * a utt_ptr that breaks its rules sets FHVAE_CB_BAD_PTR, and with that bit set nothing is written.  Every index a kernel forms
 * is re-checked against n_frames, C, the pointers and ws_bytes, so no argument makes a kernel read or write outside its buffers.
 */
#ifndef FHVAE_CTCBEAM_H
#define FHVAE_CTCBEAM_H

#include "fhvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  FHVAE_CB_BAD_PTR = 1, /* utt_ptr breaks its rules: nothing is written */
  FHVAE_CB_EMPTY = 2    /* an utterance's beam emptied out: length 0, score -inf */
};

#define FHVAE_CB_MAX_CLASSES 128 /* C above it: FHVAE_ERR_LIMIT */
#define FHVAE_CB_MAX_BEAM 64     /* W outside [1, 64]: FHVAE_ERR_LIMIT */
#define FHVAE_CB_NODE_BYTES 16   /* a trie node: parent, label, first child, next sibling */

/* bytes of trie nodes for n_frames frames at beam width W: 16 W n_frames rounded up to 256.  0 for n_frames < 0 or above 2^52
 * or W outside [1, FHVAE_CB_MAX_BEAM].  Monotone in both. */
int64_t fhvae_cb_ws_bytes(int64_t n_frames, int64_t W);

/* hyp (n_frames) int32, hyp_len (U) int32, score (U) float64.  C < 2, blank outside [0, C), n_frames, U or ws_bytes < 0,
 * ldz < C, class_beam negative or NaN, ws_bytes below fhvae_cb_ws_bytes(n_frames, W): FHVAE_ERR_SHAPE; ldz no multiple of 4,
 * logits or ws off 16 bytes, another pointer off its element: FHVAE_ERR_ALIGN; C above FHVAE_CB_MAX_CLASSES, W outside
 * [1, FHVAE_CB_MAX_BEAM], U above 2^31 - 1, n_frames above 2^52: FHVAE_ERR_LIMIT; a NULL pointer other than lm:
 * FHVAE_ERR_NULL.  U == 0: returns 0, launches nothing. */
int fhvae_cb_decode(const float* logits, int64_t ldz, int64_t n_frames, int64_t C, int64_t blank, const int64_t* utt_ptr,
                    int64_t U, int64_t W, double class_beam, const double* lm, int32_t* hyp, int32_t* hyp_len, double* score,
                    int32_t* status, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
