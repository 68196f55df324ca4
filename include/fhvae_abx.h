/*
 * fhvae_abx.h -- the hot path of the ABX phone-discrimination measure (csrc/abx.hip): the DTW distance between every two
 * tokens of a group (the tokens that share a context), for many groups in one call.  The entry point is exported from the
 * same library as include/fhvae_hip.h and follows its conventions (device pointers, enqueue only, FHVAE_ERR_* before any
 * launch); it is declared here, not there, so FHVAE_ABI_VERSION and the symbol set of that header are unchanged.
 *
 * The definitions below are this project's: nothing here runs ABXpy or the ZeroSpeech tools.
 *
 * Layout, everything on the device:
 *   feats (n_frames, D) f32, 1 <= D <= FHVAE_ABX_MAX_DIM.
 *   tok_start (N) int64, tok_len (N) int32: token i is the rows tok_start[i] .. tok_start[i] + tok_len[i] - 1 of feats,
 *     1 <= tok_len[i] <= max_len <= FHVAE_ABX_MAX_LEN.  Tokens stand in any order and may overlap.
 *   grp_ptr (G + 1) int64: the tokens arrive sorted by group; group g is the tokens grp_ptr[g] .. grp_ptr[g + 1] - 1, n_g of
 *     them (n_g = 0 is allowed).  grp_ptr[0] = 0, grp_ptr[G] = N.
 *   out_ptr (G + 1) int64: out_ptr[0] = 0, out_ptr[g + 1] - out_ptr[g] = n_g^2, out_ptr[G] = n_out.
 *   pair_ptr (G + 1) int64: pair_ptr[0] = 0, pair_ptr[g + 1] - pair_ptr[g] = n_g (n_g - 1) / 2, pair_ptr[G] = n_pairs.  It
 *     is what lets a wavefront find its pair from the flat pair index with integer comparisons only.
 *   out (n_out) f32: the block of group g, at out_ptr[g], is its dense n_g x n_g matrix of distances, row-major.  It is
 *     symmetric; its diagonal is written as 0 and is not computed.
 *
 * Frame cost of a row a of one token and a row b of another, in float64 from the f32 values, products and sums in
 * increasing k (every product of two f32 values is exact in float64, so a fused multiply-add gives the same bits):
 *     dot = sum_k a_k b_k,  na = sqrt(sum_k a_k^2),  nb = sqrt(sum_k b_k^2)
 *     cos = dot / (na * nb), clamped to [-1, 1];  cos := 0 if na = 0 or nb = 0
 *     c   = acos(cos) / pi  (FHVAE_ABX_ANGULAR)   or   1 - cos  (FHVAE_ABX_COSINE)
 *   and c is rounded once to f32.  (sqrt, the product, the division and the subtraction are correctly rounded; acos is the
 *   device library's, so a cost whose float64 value lies on an f32 rounding boundary can differ by one f32 ulp from
 *   another libm's.)
 *
 * DTW between token a (n rows) and token b (m rows), in f32 on those costs, one rounding per addition:
 *     D[0][0] = c[0][0], L[0][0] = 1;  D[0][j] = D[0][j - 1] + c[0][j];  D[i][0] = D[i - 1][0] + c[i][0]  (L likewise + 1)
 *     elsewhere the predecessor is the smallest of D[i - 1][j - 1], D[i - 1][j], D[i][j - 1], ties broken in that order
 *     (the diagonal unless the upper is strictly smaller, then the left only if it is strictly smaller than that):
 *     D[i][j] = D_pred + c[i][j],  L[i][j] = L_pred + 1
 *     d(a, b) = D[n - 1][m - 1] / (float)L[n - 1][m - 1]      (correctly rounded f32 division)
 *   the cost of the best path normalised by its length.  For tokens i < j of a group only d(token i, token j) is computed;
 *   out[j][i] is a copy.  A pair's value is a function of the two tokens alone: bitwise the same alone, inside any batch,
 *   and for any order of the groups or of the tokens.
 *
 * Status: *status is an int32 device word the library only ORs bits into; the caller clears it.  A check kernel runs first:
 * a token whose start or length breaks the rules above sets FHVAE_ABX_BAD_TOKEN; grp_ptr / out_ptr / pair_ptr that break
 * theirs set FHVAE_ABX_BAD_PTR.  With either bit set the kernels behind it write nothing.  They also re-check every index
 * they form, so no argument makes a kernel read or write outside its buffers.
 */
#ifndef FHVAE_ABX_H
#define FHVAE_ABX_H

#include "fhvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { FHVAE_ABX_ANGULAR = 0, FHVAE_ABX_COSINE = 1 }; /* metric */
enum {
  FHVAE_ABX_BAD_TOKEN = 1, /* a token's start or length is outside feats or the length limit */
  FHVAE_ABX_BAD_PTR = 2    /* grp_ptr / out_ptr / pair_ptr are not monotone, do not end at N / n_out / n_pairs, or disagree */
};

#define FHVAE_ABX_MAX_DIM 128 /* D above it: FHVAE_ERR_LIMIT */
#define FHVAE_ABX_MAX_LEN 64  /* frames of a token, at most */

/* out = the DTW distances of every group.  1 <= D (FHVAE_ERR_SHAPE) <= FHVAE_ABX_MAX_DIM (FHVAE_ERR_LIMIT); N, G, n_pairs <=
 * 2^31 - 1 (FHVAE_ERR_LIMIT); n_frames, n_pairs, n_out >= 0 and metric known (FHVAE_ERR_SHAPE).  max_len in [1,
 * FHVAE_ABX_MAX_LEN] (FHVAE_ERR_SHAPE below, FHVAE_ERR_LIMIT above) is the caller's bound on tok_len: a longer token sets
 * FHVAE_ABX_BAD_TOKEN.  It only chooses how much on-chip memory a pair is given (bounds up to 16, up to 32 and up to 64 rows
 * have an instance each, the smaller ones faster); the values do not depend on it (bitwise).  n_pairs and n_out are the host's
 * copies of pair_ptr[G] and out_ptr[G]; the check kernel compares them.  N == 0 or G == 0: returns 0, launches nothing. */
int fhvae_abx_dtw(const float* feats, int64_t n_frames, int64_t D, const int64_t* tok_start, const int32_t* tok_len, int64_t N,
                  int64_t max_len, const int64_t* grp_ptr, const int64_t* out_ptr, const int64_t* pair_ptr, int64_t G, int64_t n_pairs,
                  int64_t n_out, int metric, float* out, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
