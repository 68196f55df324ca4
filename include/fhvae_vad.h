/*
 * fhvae_vad.h -- energy voice-activity detection on the device (csrc/vad.hip): per-frame energies of a batch of waveforms,
 * the voiced / unvoiced decision of every frame with the destination of every voiced row, and the selection of the voiced
 * rows of a feature matrix.  Replaces AudioUtils.energy_vad (utils.py:275-300 of the reference, librosa 0.8.0) and stands in
 * for Kaldi's compute-vad-decision + select-voiced-frames.  The entry points are exported from the same library as
 * include/fhvae_hip.h and follow its conventions (device pointers, enqueue only, FHVAE_ERR_* before any launch); they are
 * declared here, not there, so FHVAE_ABI_VERSION and the symbol set of that header are unchanged.
 *
 * The definitions below are this project's: nothing here runs librosa or a Kaldi binary.
 *
 * Batch layout (that of fhvae_feats_fwd / fhvae_kaldi_fbank_fwd): wave (n_samples) f32, the utterances' samples
 * concatenated; wave_ptr (U + 1) int64 their offsets; frame_ptr (U + 1) int64 the offsets of their frames, frame_ptr[0] = 0,
 * frame_ptr[U] = n_frames.  All on the device.
 *
 * Energy, L = frame_len, hop = frame_shift, an utterance of n samples x[0 .. n - 1]:
 *   FHVAE_VAD_RMS_CENTER  librosa.feature.rms(y, frame_length=L, hop_length=hop, center=True, pad_mode="reflect") (`rmse`,
 *     which the reference calls, is the older name of the same function).  Samples at full scale 1.0, no pre-emphasis.  The
 *     utterance is padded by L / 2 on both sides by reflection, the edge not repeated: padded position p stands for
 *     i = p - L / 2, and reads x[-i] for i < 0, x[2 (n - 1) - i] for i >= n.  Frame f covers padded positions f hop ..
 *     f hop + L - 1;  e = sqrt(sum x^2 / L).  Frames: 1 + (n + 2 (L / 2) - L) / hop, what fhvae_feats_fwd counts; n >= L / 2 + 1
 *     (one reflection suffices).  Any L >= 2, odd ones included.
 *   FHVAE_VAD_LOGE_SNIP   Kaldi's raw log energy (compute-mfcc-feats --use-energy=true --raw-energy=true, snip-edges): frame f
 *     covers samples f hop .. f hop + L - 1 on Kaldi's int16 scale (the caller uploads the samples times 32768); with the
 *     flag FHVAE_VAD_REMOVE_DC the frame's mean is subtracted first;  e = ln(max(sum x^2, FLT_EPSILON)).  No pre-emphasis,
 *     no window, and NO DITHER: in the Kaldi recipes the MFCCs behind the VAD come from a run of their own, whose dither is
 *     a separate, unrepeatable rand() draw, so an energy that is independent of the noise added to the fbank features is the
 *     faithful choice.  Frames: 0 for n < L, else 1 + (n - L) / hop; n >= L.
 *   Arithmetic: the squares, the frame's sum, the DC mean, the division, sqrt and ln are float64; the result is rounded
 *   once to f32 and stored.  The order of the sum is fixed and a function of the frame alone (lane j of 16 adds positions j,
 *   j + 16, ... in increasing order; the 16 partial sums are combined by a fixed butterfly), so a frame's energy does not
 *   depend on the batch (bitwise).
 *
 * Decision, one formula for both conventions, everything in float64 from the STORED f32 energies; T_u the frames of
 * utterance u, t a frame of it:
 *     th[u]  = thr_abs + mean_scale * ((sum of e over utterance u) / T_u)
 *     a[t]   = e[t] > th[u]
 *     num(t) = #{t2 in [t - ctx, t + ctx] and [0, T_u) : a[t2]},  den(t) = the size of that range
 *     vad[t] = (float)num >= (float)den * proportion               (f32, one rounding; uint8 0 / 1)
 *   The reference is thr_abs = 0, mean_scale = th_ratio (default 1.04 / 2), ctx = 0, any proportion in (0, 1].  Kaldi's
 *   ComputeVadEnergy has --vad-energy-threshold (thr_abs), --vad-energy-mean-scale, --vad-frames-context (ctx) and
 *   --vad-proportion-threshold, which this project takes to default to 5.0, 0.5, 0 and 0.6.  The context never crosses an
 *   utterance boundary.  The utterance's sum is float64 without floating-point atomics, in an order defined relative to the
 *   utterance's first frame: one partial per chunk of FHVAE_VAD_CHUNK frames of the utterance (thread j of 256 adds frames j,
 *   j + 256, ... of the chunk, the 256 sums are combined by a fixed tree), then the chunks in order; an utterance's decisions
 *   are bitwise the same alone or inside any batch, and a long utterance is summed by as many workgroups as it has chunks.
 *   rank (n_frames + 1) int64 is the exclusive prefix count of vad over the whole batch (integer scan in three phases over
 *   tiles of FHVAE_VAD_TILE frames): rank[r] is the destination row of a voiced frame r, rank[frame_ptr[u + 1]] -
 *   rank[frame_ptr[u]] the voiced frames of utterance u, rank[n_frames] their total.
 *
 * Selection (select-voiced-frames): out[rank[r], :] = rows[r, :] for every r with vad[r] = 1; a copy, bitwise.
 *
 * Status: *status is an int32 device word the library only ORs bits into; the caller clears it.  frame_ptr / wave_ptr that
 * break the rules above (every utterance has at least one frame and exactly the frames its samples give) set
 * FHVAE_VAD_BAD_PTR and nothing is written; a vad / rank pair that does not belong together sets FHVAE_VAD_BAD_RANK in
 * fhvae_vad_select and the rows concerned are written as zeros.  No argument makes a kernel read or write outside its
 * buffers.
 */
#ifndef FHVAE_VAD_H
#define FHVAE_VAD_H

#include "fhvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { FHVAE_VAD_RMS_CENTER = 0, FHVAE_VAD_LOGE_SNIP = 1 }; /* mode */
enum { FHVAE_VAD_REMOVE_DC = 1 };                           /* flags (FHVAE_VAD_LOGE_SNIP only) */
enum {
  FHVAE_VAD_BAD_PTR = 1, /* wave_ptr / frame_ptr break the framing rule */
  FHVAE_VAD_BAD_RANK = 2 /* select: rank is not the exclusive prefix count of vad */
};

#define FHVAE_VAD_MAX_FRAME 4096 /* frame_len above it: FHVAE_ERR_LIMIT */
#define FHVAE_VAD_MAX_CTX 1024   /* ctx above it: FHVAE_ERR_LIMIT */
#define FHVAE_VAD_CHUNK 1024     /* frames per partial sum of an utterance's mean */
#define FHVAE_VAD_TILE 1024      /* frames per tile of the prefix count */

/* energy (n_frames) f32 of the batch.  frame_len in [2, FHVAE_VAD_MAX_FRAME] (FHVAE_ERR_SHAPE below, FHVAE_ERR_LIMIT
 * above), frame_shift >= 1, mode and flags as above (FHVAE_ERR_SHAPE for unknown ones).  n_frames == 0: returns 0,
 * launches nothing. */
int fhvae_vad_energy(const float* wave, int64_t n_samples, const int64_t* wave_ptr, const int64_t* frame_ptr, int64_t U,
                     int64_t n_frames, int64_t frame_len, int64_t frame_shift, int mode, int flags, float* energy,
                     int32_t* status, void* stream);

/* Bytes of the workspace fhvae_vad_decide needs for n_frames frames in U utterances (the chunk partials, the thresholds, the
 * tile counts); < 0: FHVAE_ERR_* for negative sizes. */
int64_t fhvae_vad_ws_bytes(int64_t n_frames, int64_t U);

/* vad (n_frames) uint8 and rank (n_frames + 1) int64 from energy (n_frames) f32, which may come from anywhere (a C0 column
 * read from an archive, say).  ws: ws_bytes >= fhvae_vad_ws_bytes(n_frames, U) bytes, 8-byte aligned (FHVAE_ERR_SHAPE /
 * FHVAE_ERR_ALIGN); its contents before and after the call mean nothing.  0 <= ctx <= FHVAE_VAD_MAX_CTX; proportion in
 * (0, 1]; thr_abs and mean_scale finite.  n_frames == 0: returns 0, launches nothing. */
int fhvae_vad_decide(const float* energy, const int64_t* frame_ptr, int64_t U, int64_t n_frames, double thr_abs,
                     double mean_scale, int64_t ctx, float proportion, void* ws, int64_t ws_bytes, uint8_t* vad, int64_t* rank,
                     int32_t* status, void* stream);

/* out (n_out, F) f32 = the rows of rows (n_frames, F) with vad = 1, n_out = rank[n_frames] as the caller read it.  A gather
 * per output row: row j finds the last r with rank[r] <= j; unless vad[r] = 1 and rank[r] = j it is written as zeros and
 * FHVAE_VAD_BAD_RANK is set.  0 <= n_out <= n_frames.  n_out == 0: returns 0, launches nothing. */
int fhvae_vad_select(const float* rows, const uint8_t* vad, const int64_t* rank, int64_t n_frames, int64_t F, int64_t n_out,
                     float* out, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
