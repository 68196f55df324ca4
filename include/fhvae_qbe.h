/*
 * fhvae_qbe.h -- the hot path of query-by-example search on frame-level features (csrc/qbe.hip): subsequence DTW of every
 * query against every utterance, with a free start and a free end in the utterance, for a whole Q x U grid in one call.  The
 * entry point is exported from the same library as include/fhvae_hip.h and follows its conventions (device pointers, enqueue
 * only, FHVAE_ERR_* before any launch); it is declared here, not there, so FHVAE_ABI_VERSION and the symbol set of that header
 * are unchanged.
 *
 * The definitions below are this project's: nothing here runs an external query-by-example tool.
 *
 * Layout, everything on the device:
 *   qfeats (nq_frames, D) f32 with q_start (Q) int64 and q_len (Q) int32: query k is the rows q_start[k] .. q_start[k] +
 *     q_len[k] - 1 of qfeats, 1 <= q_len[k] <= max_qlen <= FHVAE_QBE_MAX_QLEN.  Queries stand in any order and may overlap.
 *   feats (n_frames, D) f32 with utt_ptr (U + 1) int64: utterance u is the rows utt_ptr[u] .. utt_ptr[u + 1] - 1 of feats.
 *     utt_ptr is monotone, utt_ptr[0] = 0, utt_ptr[U] = n_frames; an utterance may be empty and holds at most 2^31 - 1 frames.
 *   qfeats and feats may be the same pointer.  Rows are contiguous (no leading dimension).  1 <= D <= FHVAE_QBE_MAX_DIM.
 *
 * Frame cost c[i][j] of query row i and utterance frame j: the frame cost of include/fhvae_abx.h, to the letter (float64 dot
 * and norms summed in increasing k, the cosine clamped and 0 against a zero row, acos / pi for FHVAE_QBE_ANGULAR or 1 - cos for
 * FHVAE_QBE_COSINE, rounded once to f32; the metric codes are those of FHVAE_ABX_*).
 *
 * Recursion for a query of n rows and an utterance of m >= 1 frames (m < n is allowed), in f32, one rounding per addition.
 * D is the cost of the best path that ends in (i, j), L its number of cells, S the utterance frame it started at:
 *     D[0][j] = c[0][j]                 L[0][j] = 1              S[0][j] = j        (the start is free)
 *     D[i][0] = D[i-1][0] + c[i][0]     L[i][0] = L[i-1][0] + 1  S[i][0] = S[i-1][0]
 *     elsewhere the predecessor is the smallest of D[i-1][j-1], D[i-1][j], D[i][j-1], ties broken in that order (the diagonal
 *     unless the upper is strictly smaller, then the left only if it is strictly smaller than that), as in fhvae_abx.h:
 *     D[i][j] = D_pred + c[i][j]        L[i][j] = L_pred + 1     S[i][j] = S_pred
 *     e[j] = D[n-1][j] / (float)L[n-1][j]      (correctly rounded f32 division)          s[j] = S[n-1][j]
 *   e[j] is the length-normalised cost of the best alignment of the whole query that ends at frame j, s[j] where it starts.
 *   For every j, e[j] equals the fhvae_abx.h distance d(query, frames s[j] .. j) whenever that alignment is the unique best.
 *
 * Outputs:
 *   best_cost (Q, U) f32, best_start (Q, U) int32, best_end (Q, U) int32: best_end is the smallest j that minimises e[j],
 *     best_cost = e[best_end], best_start = s[best_end]; frames count from the utterance's start.  An empty utterance gives
 *     +inf, -1, -1.  (An e[j] that is NaN never wins; an utterance whose every e[j] is NaN gives +inf, -1, -1 too.)
 *   end_cost (Q, n_frames) f32 and end_start (Q, n_frames) int32, each optional (NULL: not written): the whole profile, e[j]
 *     and s[j] of utterance u at column utt_ptr[u] + j.
 *   The result of a (query, utterance) cell is a function of those two alone: bitwise the same alone, inside any batch, for
 *   any max_qlen and for whatever column tile the kernel walks the utterance in.
 *
 * Status: *status is an int32 device word the library only ORs bits into; the caller clears it.  A check kernel runs first:
 * a query whose start or length breaks the rules above sets FHVAE_QBE_BAD_QUERY; utt_ptr that breaks its rules sets
 * FHVAE_QBE_BAD_PTR.  With either bit set the kernel behind it writes nothing.  It also re-checks every index it forms, so no
 * argument makes a kernel read or write outside its buffers.
 */
#ifndef FHVAE_QBE_H
#define FHVAE_QBE_H

#include "fhvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { FHVAE_QBE_ANGULAR = 0, FHVAE_QBE_COSINE = 1 }; /* metric: the codes of FHVAE_ABX_* */
enum {
  FHVAE_QBE_BAD_QUERY = 1, /* a query's start or length is outside qfeats or the length limit */
  FHVAE_QBE_BAD_PTR = 2    /* utt_ptr is not monotone, does not run from 0 to n_frames, or an utterance is too long */
};

#define FHVAE_QBE_MAX_DIM 128 /* D above it: FHVAE_ERR_LIMIT */
#define FHVAE_QBE_MAX_QLEN 64 /* frames of a query, at most */

/* The Q x U grid.  1 <= D (FHVAE_ERR_SHAPE) <= FHVAE_QBE_MAX_DIM (FHVAE_ERR_LIMIT); nq_frames, n_frames, Q, U >= 0 and metric
 * known (FHVAE_ERR_SHAPE); Q * U <= 2^31 - 1, and Q * n_frames below 2^63 when a profile is asked for (FHVAE_ERR_LIMIT).
 * max_qlen in [1, FHVAE_QBE_MAX_QLEN] (FHVAE_ERR_SHAPE below, FHVAE_ERR_LIMIT above) is the caller's bound on q_len: a longer
 * query sets FHVAE_QBE_BAD_QUERY.  It only chooses how much on-chip memory a cell is given (bounds up to 16, up to 32 and up to
 * 64 rows have an instance each, the smaller ones faster); the values do not depend on it (bitwise).  end_cost and end_start
 * may be NULL.  Q == 0 or U == 0: returns 0, launches nothing. */
int fhvae_qbe_sdtw(const float* qfeats, int64_t nq_frames, const float* feats, int64_t n_frames, int64_t D, const int64_t* q_start,
                   const int32_t* q_len, int64_t Q, int64_t max_qlen, const int64_t* utt_ptr, int64_t U, int metric, float* best_cost,
                   int32_t* best_start, int32_t* best_end, float* end_cost, int32_t* end_start, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
