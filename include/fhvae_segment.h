/*
 * fhvae_segment.h -- segmentation of an utterance into units of a codebook (csrc/segment.hip): the cut into segments of at most
 * Lmax frames, and the unit of every segment, that minimise the quantisation error plus a penalty per segment (a dynamic
 * programme over the codebook; "DPDP" in the unit-discovery literature).  The entry points are exported from the same library
 * as include/fhvae_hip.h and follow its conventions (device pointers, enqueue only, FHVAE_ERR_* before any launch); they are
 * declared here, not there, so FHVAE_ABI_VERSION and the symbol set of that header are unchanged.
 *
 * The definitions below are this project's: no reference implementation is run or compared with.
 *
 * An utterance has frames x_0 .. x_{T-1} of D f32 values; the codebook is c_k, (K, D); 1 <= Lmax <= FHVAE_SEG_MAX_LEN is the
 * longest segment in frames and lambda >= 0 a float64 penalty per segment.  Over all cuts into segments of 1 .. Lmax frames,
 *     J = sum over the segments [ min_k sum_{f in seg} |x_f - c_k|^2 + lambda ]
 * sum_f |x_f|^2 is the same for every cut and is dropped: with S = sum_{f in seg} x_f and l the segment's length, the score of
 * unit k is l |c_k|^2 - 2 S . c_k.  (A length penalty -w (l - 1) differs from lambda = w per segment by the constant w T alone;
 * lambda is the only form built.)
 *
 * Layout, everything on the device:
 *   x     (n_frames, D) f32, leading dimension ldx; cent (K, D) f32, leading dimension ldc: the rules of include/fhvae_kmeans.h
 *         (D a multiple of 16 in [16, 128], leading dimensions multiples of 4 and at least D, 16-byte aligned pointers),
 *         1 <= n_frames <= FHVAE_KM_MAX_ROWS, 1 <= K <= FHVAE_KM_MAX_CENT.
 *   utt_ptr (U + 1) int64: utterance u is the rows utt_ptr[u] .. utt_ptr[u + 1] - 1; monotone, utt_ptr[0] = 0, utt_ptr[U] =
 *         n_frames.  An utterance may be empty.
 *   ws    fhvae_seg_ws_bytes(n_frames, K, D, Lmax) bytes, 16-byte aligned.  Both calls use it; nothing in it outlives a call.
 *
 * PHASE 1 (fhvae_seg_scores).  A cell is a global row n, the LAST frame of a segment, and a length l = 1 .. Lmax: the segment is
 * the rows n - l + 1 .. n.
 *     S64(n, l)[d] = the float64 sum of (double)x[n][d], x[n-1][d], .. x[n-l+1][d], in that order, from 0
 *                    (so S64(n, l) is S64(n, l - 1) plus one addition);  Sf = (float)S64, one rounding
 *     cn[k]        = sum_d c[k][d]^2, the fmaf chain of include/fhvae_kmeans.h
 *     dot(n, l, k) = Sf(n, l) . c[k], the dot of csrc/allpairs_f32.h in its documented order
 *     s(n, l, k)   = fmaf(-2, dot, (float)l * cn[k])            (the product rounded once)
 *     score[n][l-1] = min_k s(n, l, k);  unit[n][l-1] = the smallest k that attains it
 *   A score that is NaN never wins; a cell whose every score is NaN has score +inf and unit 0 (as fhvae_km_assign's label 0).
 *   A segment that would begin before its utterance's first row has score +inf and unit -1.  A cell is a function of the
 *   utterance's rows and the table alone: bitwise the same alone, in any batch and at any position of a workgroup's tile.  The
 *   segment sums are built FHVAE_SEG_CHUNK_ROWS rows at a time into ws: no (n_frames Lmax, D) array exists for the whole call.
 *
 * PHASE 2 (fhvae_seg_dp).  Per utterance of T rows from row r0 on, in float64 with one rounding per addition:
 *     alpha[0] = 0
 *     alpha[t] = min over 1 <= l <= min(Lmax, t) of ( alpha[t - l] + (double)score[r0 + t - 1][l - 1] ) + lambda
 *     back[t]  = the smallest l that attains the minimum
 *   A candidate that is +inf or NaN never wins (with nothing else, alpha[t] = +inf and back[t] = 1).  cost[u] = alpha[T].  The
 *   walk from T along back gives the segments; for every frame n, seg_unit[n] is unit[last row of its segment][l - 1] and
 *   seg_start[n] is 1 on the first frame of a segment, else 0; n_seg[u] counts the segments.  An utterance with T = 0 has
 *   n_seg 0 and cost 0.  An utterance whose alpha[T] is not finite (a NaN row does that) sets FHVAE_SEG_NOT_FINITE and gets
 *   nothing written: neither cost nor n_seg nor its rows of seg_unit and seg_start.  It concerns that utterance only.
 *   An utterance's outputs are a function of its rows of score and unit alone: the same bits alone and in any batch.
 *
 * Status: *status is an int32 device word the library only ORs bits into; the caller clears it.  A check kernel runs first in
 * both calls: a utt_ptr that breaks its rules sets FHVAE_SEG_BAD_PTR, and with that bit set the kernels behind it write
 * nothing.  Every kernel re-checks each index it forms, and a back-pointer read in the trace-back is clamped, so no argument
 * makes a kernel read or write outside its buffers.
 */
#ifndef FHVAE_SEGMENT_H
#define FHVAE_SEGMENT_H

#include "fhvae_kmeans.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  FHVAE_SEG_BAD_PTR = 1,   /* utt_ptr is not monotone or does not run from 0 to n_frames: nothing is written */
  FHVAE_SEG_NOT_FINITE = 2 /* an utterance's alpha[T] is not finite: nothing is written for it */
};

#define FHVAE_SEG_MAX_LEN 64       /* Lmax outside [1, 64]: FHVAE_ERR_LIMIT (a wavefront's lane per length) */
#define FHVAE_SEG_CHUNK_ROWS 4096  /* rows whose segment sums are in ws at a time */

/* bytes of workspace; 0 for arguments the calls below refuse.  Monotone in each argument. */
int64_t fhvae_seg_ws_bytes(int64_t n_frames, int64_t K, int64_t D, int64_t Lmax);

/* score (n_frames, Lmax) f32, unit (n_frames, Lmax) int32, status (1) int32.  n_frames, K, U < 1, a D or a leading dimension
 * the all-pairs pass does not take, ws_bytes below fhvae_seg_ws_bytes: FHVAE_ERR_SHAPE; a pointer or leading dimension off its
 * alignment: FHVAE_ERR_ALIGN; n_frames or K above the k-means limits, Lmax outside [1, FHVAE_SEG_MAX_LEN], U above 2^31 - 1:
 * FHVAE_ERR_LIMIT. */
int fhvae_seg_scores(const float* x, int64_t ldx, int64_t n_frames, int64_t D, const float* cent, int64_t ldc, int64_t K,
                     int64_t Lmax, const int64_t* utt_ptr, int64_t U, void* ws, int64_t ws_bytes, float* score, int32_t* unit,
                     int32_t* status, void* stream);

/* score and unit as above (dense, leading dimension Lmax), seg_unit (n_frames) int32, seg_start (n_frames) uint8, n_seg (U)
 * int32, cost (U) float64.  ws holds one back-pointer byte per row: ws_bytes >= n_frames (any fhvae_seg_ws_bytes is enough).
 * n_frames < 0, U < 1, a lambda that is negative or NaN, ws_bytes < n_frames: FHVAE_ERR_SHAPE; the alignments and limits of
 * fhvae_seg_scores. */
int fhvae_seg_dp(const float* score, const int32_t* unit, int64_t n_frames, int64_t Lmax, const int64_t* utt_ptr, int64_t U,
                 double lambda, void* ws, int64_t ws_bytes, int32_t* seg_unit, uint8_t* seg_start, int32_t* n_seg, double* cost,
                 int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
