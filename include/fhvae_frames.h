/*
 * fhvae_frames.h -- the frame-level entry points of libfhvae_hip.so (csrc/frames.hip): dense, edge-replicated windows cut
 * from a resident corpus, and the inverse overlap average.  They are exported from the same library as include/fhvae_hip.h
 * and follow its conventions (device pointers, enqueue only, FHVAE_ERR_* before any launch); they are declared here, not
 * there, so FHVAE_ABI_VERSION and the symbol set of that header are unchanged.
 *
 * Geometry ("Frame-level latents").  An utterance has n >= 1 frames, the model T frames per segment,
 * left = T / 2.  With window shift s >= 1 the utterance has W = ceil(n / s) windows; window k is centred on frame k s:
 * position t of window k stands for local frame p = k s - left + t and reads frame min(max(p, 0), n - 1) (edge
 * replication).  The corpus is the concatenation of its U utterances: utt_ptr (U + 1) holds frame offsets and win_ptr
 * (U + 1) window offsets, both int64 on the device, both starting at 0; global window w is window w - win_ptr[u] of the
 * utterance u with win_ptr[u] <= w < win_ptr[u + 1].  The CSR rule every kernel re-checks for the utterance it touches:
 *     win_ptr[u + 1] - win_ptr[u] == ceil((utt_ptr[u + 1] - utt_ptr[u]) / s),  utt_ptr[u + 1] > utt_ptr[u] >= 0
 * (fhvae_frames_gather: also utt_ptr[u + 1] <= pool_frames).  A window or frame whose utterance breaks it, or that lies in
 * no utterance, is written as zeros and sets FHVAE_FRAMES_BAD_PTR in *status; no argument makes a kernel read or write
 * outside its buffers.  The library only ever ORs bits into *status; the caller clears it.
 *
 * Arithmetic: f32, one rounding per operation (no fused multiply-add), correctly rounded division.
 */
#ifndef FHVAE_FRAMES_H
#define FHVAE_FRAMES_H

#include "fhvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  FHVAE_FRAMES_BAD_PTR = 1,   /* utt_ptr / win_ptr break the CSR rule for a touched utterance */
  FHVAE_FRAMES_BAD_RANGE = 2  /* overlap_mean: a frame has a covering window outside [w0, w0 + B) */
};

/* Windows [w0, w0 + B) of the corpus out of pool (pool_frames, F) f32, batch-major into out_btf (B, T, F) and / or
 * time-major into out_tbf (T, B, F) (at least one non-NULL), as (x - mean[f]) * inv_std[f] when mean and inv_std (F,) are
 * both given (both or neither).  Any shift >= 1.  Each thread finds its utterance by binary search in win_ptr.
 * B == 0: returns 0, launches nothing. */
int fhvae_frames_gather(const float* pool, int64_t pool_frames, const int64_t* utt_ptr, const int64_t* win_ptr, int64_t U,
                        int64_t w0, int64_t B, int64_t T, int64_t F, int64_t shift, const float* mean, const float* inv_std,
                        float* out_btf, float* out_tbf, int32_t* status, void* stream);

/* The overlap mean of per-window values seg (B, T, F), the windows [w0, w0 + B), for corpus frames [g0, g0 + G) into out
 * (G, F).  Local frame f of an utterance is covered by its windows k0 .. k1,
 *     k0 = max(0, ceil((f + left - T + 1) / shift)),  k1 = min(W - 1, floor((f + left) / shift));
 * out = (v[k0] + v[k0 + 1] + ... + v[k1]) / (k1 - k0 + 1) with v[k] = seg[k, f + left - k shift, :], summed in that order,
 * then out * std[f] + mean[f] when mean and std (F,) are both given.  A gather: no atomics, bitwise reproducible.
 * Needs 1 <= shift <= T - T / 2 (every frame is covered): FHVAE_ERR_SHAPE otherwise.  A frame with a covering window
 * outside [w0, w0 + B) is written as zeros and sets FHVAE_FRAMES_BAD_RANGE.  G == 0: returns 0, launches nothing. */
int fhvae_frames_overlap_mean(const float* seg, int64_t w0, int64_t B, const int64_t* utt_ptr, const int64_t* win_ptr, int64_t U,
                              int64_t g0, int64_t G, int64_t T, int64_t F, int64_t shift, const float* mean, const float* std,
                              float* out, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
