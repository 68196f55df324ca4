/*
 * fhvae_kmeans.h -- k-means on frame-level latents (csrc/kmeans.hip): the assignment of every row to its nearest centroid and
 * the centroid update, the two halves of a Lloyd iteration.  The entry points are exported from the same library as
 * include/fhvae_hip.h and follow its conventions (device pointers, enqueue only, FHVAE_ERR_* before any launch); they are
 * declared here, not there, so FHVAE_ABI_VERSION and the symbol set of that header are unchanged.
 *
 * The definitions below are this project's: nothing here runs scikit-learn or faiss.
 *
 * Layout, everything on the device:
 *   x    (N, D) f32, leading dimension ldx;  cent (K, D) f32, leading dimension ldc.  D a multiple of 16 in [16, 128], the
 *        leading dimensions multiples of 4 and at least D, the pointers 16-byte aligned (the rules of the all-pairs pass,
 *        csrc/allpairs_f32.h).  1 <= N <= FHVAE_KM_MAX_ROWS, 1 <= K <= FHVAE_KM_MAX_CENT.
 *   ws   fhvae_km_ws_bytes(N, K, D) bytes, 16-byte aligned.  Both calls use it; nothing in it outlives a call.
 *
 * ASSIGNMENT (fhvae_km_assign), all in f32:
 *     cn[k]    = sum_d c[k][d]^2,  xn[n] = sum_d x[n][d]^2     one fmaf chain each, in increasing d, from 0
 *     dot(n,k) = x[n] . c[k]                                  the dot of csrc/allpairs_f32.h, in its documented order
 *     s(n, k)  = fmaf(-2, dot(n, k), cn[k])                   (|x - c|^2 without the row's own xn: the same k wins)
 *     assign[n] = the k with the smallest s(n, k); equal scores go to the smallest k
 *     dist[n]   = fmaxf(xn[n] + s(n, assign[n]), 0)           one rounding for the sum
 *   A row's result is a function of that row and the centroid table alone: bitwise the same alone, in any batch and at any
 *   position of a workgroup's tile of 256 rows.  Two bitwise equal centroid rows give bitwise equal scores.  A score that is
 *   NaN never wins; a row whose every score is NaN (or +inf) gets label 0.
 *
 * UPDATE (fhvae_km_update).  The members of cluster k are the rows perm[cl_ptr[k] .. cl_ptr[k + 1] - 1], in the order the
 * caller lists them (increasing row index, if the result is to be a function of the labels alone: a stable sort of the labels
 * gives perm, a prefix of the counts cl_ptr).  cl_ptr[0] = 0, cl_ptr[K] = N, count[k] = cl_ptr[k + 1] - cl_ptr[k].  Cut
 * the members of a cluster into pieces of FHVAE_KM_PIECE consecutive members (the last one shorter).  In float64:
 *     piece[j][d] = sum over the piece's members, in member order, from 0, of (double)x[member][d]
 *     sum[d]      = sum over j, in piece order, from 0, of piece[j][d]
 *     cent[k][d]  = (float)(sum[d] / (double)count[k])        a correctly rounded division, one rounding to f32
 *   cl_inertia[k] is the same two-level float64 sum over (double)dist[member], not divided.  A cluster without members keeps
 *   its centroid and gets count 0 and inertia 0.  No floating-point atomics: the result depends on the members and their
 *   order alone, not on the grid, on K or on what else the call holds.
 *
 * Status: *status is an int32 device word the library only ORs bits into; the caller clears it.  A check kernel runs first:
 * cl_ptr that is not monotone or does not run from 0 to N sets FHVAE_KM_BAD_PTR, a perm entry outside [0, N) sets
 * FHVAE_KM_BAD_PERM.  With either bit set the kernels behind it write nothing.  They also re-check every index they form, so
 * no argument makes a kernel read or write outside its buffers.
 */
#ifndef FHVAE_KMEANS_H
#define FHVAE_KMEANS_H

#include "fhvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  FHVAE_KM_BAD_PTR = 1, /* cl_ptr is not monotone or does not run from 0 to N */
  FHVAE_KM_BAD_PERM = 2 /* a perm entry lies outside [0, N) */
};

#define FHVAE_KM_PIECE 256          /* members per piece of the update's two-level sum */
#define FHVAE_KM_MAX_ROWS 1073741824 /* N above 2^30: FHVAE_ERR_LIMIT */
#define FHVAE_KM_MAX_CENT 1048576    /* K above 2^20: FHVAE_ERR_LIMIT */

/* bytes of workspace for N rows, K centroids of D values; 0 for arguments the calls below refuse.  Monotone in N and in K. */
int64_t fhvae_km_ws_bytes(int64_t N, int64_t K, int64_t D);

/* assign (N) int32, dist (N) f32 or NULL.  N, K < 1 and a D or a leading dimension the all-pairs pass does not take:
 * FHVAE_ERR_SHAPE; a pointer or leading dimension off its alignment: FHVAE_ERR_ALIGN; N, K above their limits:
 * FHVAE_ERR_LIMIT; ws_bytes below fhvae_km_ws_bytes(N, K, D): FHVAE_ERR_SHAPE. */
int fhvae_km_assign(const float* x, int64_t ldx, int64_t N, int64_t D, const float* cent, int64_t ldc, int64_t K, void* ws,
                    int64_t ws_bytes, int32_t* assign, float* dist, void* stream);

/* perm (N) int64, cl_ptr (K + 1) int64, dist (N) f32 or NULL, cent (K, D) in / out, count (K) int64, cl_inertia (K) float64 or
 * NULL (written as 0 when dist is NULL), status (1) int32.  The argument errors of fhvae_km_assign. */
int fhvae_km_update(const float* x, int64_t ldx, int64_t N, int64_t D, const int64_t* perm, const int64_t* cl_ptr, int64_t K,
                    const float* dist, void* ws, int64_t ws_bytes, float* cent, int64_t ldc, int64_t* count, double* cl_inertia,
                    int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
