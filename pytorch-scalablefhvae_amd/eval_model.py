"""eval_model.py -- what the reference's eval_model.py leaves as TODOs (eval_model.py:57-59: load data, evaluate, visualise):
load a checkpoint, then write as .npy files under --out

  z1_mu.npy, z2_mu.npy        per-segment posterior means (model.encode)
  seq_ids.npy                 the sequence index of every segment
  mu2.npy, mu2_seqs.npy       the closed-form per-sequence mu2 (utils.estimate_mu2_dict) and the sequences it covers
  recon_x.npy, recon_mu.npy, recon_logvar.npy   the first --max-recon segments and model.reconstruct of them
  convert_mu.npy, convert_logvar.npy            with --convert-to Y: those segments decoded with sequence Y's mu2
  summary.json                the mean lower bound per frame over the data (forward() with zero noise: the ELBO at the
                              posterior means), segment / sequence counts

With --wav-out DIR --wav-seqs N (needs --feat-scp data of "spec" features, n_fft // 2 + 1 columns for --sr / --win-t) the first N
sequences are also made audible: every segment of a sequence is reconstructed (and, with --convert-to Y, decoded with Y's
mu2), the decoder means are un-normalised, put back together (utils.overlap_mean) and turned into a waveform by Griffin-Lim
(features.synthesize): DIR/<seq>_orig.wav (the input features through the same vocoder: the ceiling of what it can do),
<seq>_recon.wav and <seq>_to_<Y>.wav, listed under "wavs" in summary.json.  With --wav-ftype fbank the data are mel features
(as many columns as the checkpoint's feature width) and the three go through features.synthesize_mel instead: linear
magnitudes fitted to the mel magnitudes (non-negative least squares, --nnls-iters steps), then the same Griffin-Lim.

With --utt2spk FILE (Kaldi's `<seq> <spk>` lines) or --spk-key-sep SEP (the speaker is the sequence key up to the first SEP: "-"
for preprocess_librispeech.py's ids, "_" for preprocess_timit.py's; both need --feat-scp data) the factorization is measured by
speaker verification (verification.py): every sequence against every other by the cosine of their mu2 (the rows of mu2.npy) and,
as the control, of their z1_mean (the mean of the sequence's segments' z1_mu); summary.json gains "speaker_verification" with the
equal error rate of both, and sv_hist_mu2.npy / sv_hist_z1_mean.npy hold the (2, --sv-bins) target / non-target score histograms
(a DET curve can be drawn from them).  A factorized model gives a low EER on mu2 and a high one on z1_mean.
With --sv-backend lda and / or plda (spk_backend.py; --sv-train-feat-scp / --sv-train-len-scp name the training sequences, whose
speakers follow the same --utt2spk / --spk-key-sep rule; --sv-lda-dim K, --sv-plda-iters N, --sv-no-length-norm) a back end is
trained on the training sequences' embeddings and both entries gain "lda" (the cosine after the LDA) and / or "plda" (the PLDA
log-likelihood ratio): eer, threshold, min_dcf, crossing_mass, n_target, n_nontarget, lo, hi; sv_hist_<name>_<backend>.npy and
sv_backend_<name>.npz are written.  Without it, or with cosine alone, every output is what it was.
With --sv-snorm (and a trained back end) each of these entries gains a "snorm" block: the same scores normalised against the
speakers' means of the training sequences, adaptive S-norm with the --sv-snorm-top largest cohort scores (score_norm.py; 0: the
whole cohort), and sv_hist_<name>_<backend>_snorm.npy.

With --tsne (needs --feat-scp data; --tsne-perplexity, --tsne-iters, --tsne-seed) the same two embeddings are also drawn: exact
t-SNE maps (tsne.py) go to tsne_mu2.npy and tsne_z1_mean.npy, both (sequences, 2), and to tsne.tsv, one line per sequence: the
key, the speaker (or "-"), the mu2 and the z1_mean coordinates; summary.json gains "tsne" with the perplexity, the iterations,
the seed and the final KL divergence of both maps.  With the speakers known (--utt2spk / --spk-key-sep) and matplotlib
importable, tsne_mu2.png and tsne_z1_mean.png are scatter plots with one colour per speaker: one island per speaker on mu2 and
none on z1_mean is what a factorized model shows.

With --abx-item FILE (a ZeroSpeech / ABXpy .item file, abx.read_items; needs --feat-scp data) the other half of the factorization
is measured: the ABX phone discrimination error (abx.py) of the frame-level z1 -- frames.encode_frames over every utterance at
shift 1, one row per frame -- and, as the baseline, of the normalised input features.  A token's frames are those whose time
--abx-frame-offset + f * --abx-frame-shift lies in [onset, offset].  summary.json gains "abx": {"z1": {within, across,
cells_within, cells_across, triples_within, triples_across}, "feats": {...}, "tokens", "dropped", "distance", "frame_shift",
"frame_offset"} (--abx-on chooses which of the two), and abx_by_pair_<on>.tsv lists every ordered phone pair with its within-
and across-speaker score.  A z1 that keeps the phone and loses the speaker scores below the features, most of all across speakers.

With --units K (needs --feat-scp data) the frames are turned into discrete units (units.py): a k-means codebook of K centroids
fitted on the frame-level z1 and, as the baseline, on the normalised input features (--units-on chooses; --units-iters,
--units-seed), one unit per frame.  units_<on>.txt holds one line `key u0 u1 ...` per utterance, units_centroids_<on>.npy the
codebook, and summary.json gains "units": {"z1": {on, k, frames, iterations, converged, inertia, reseeded, seed, bitrate,
bitrate_collapsed}, "feats": {...}}; --units-segment [--units-dur-penalty LAMBDA] [--units-max-seg-frames L] adds the
duration-penalised segmentation over each codebook (segment.py): segments_<on>.item, segments_<on>.txt (one unit per segment) and
a "segments" entry in each block; with --units-item FILE (a .item phone alignment; the frame grid is --abx-frame-shift /
--abx-frame-offset) every sub-block also holds cluster_purity, phone_purity, pnmi, labelled_frames, overlaps and phones.

With --qbe-queries ITEM --qbe-item ITEM (needs --feat-scp data) spoken terms are searched for by example (qbe.py): the queries are
the first --qbe-max-per-term tokens of every term of ITEM (the #phone column is the term; tokens of at most 64 frames), each is
aligned against every other utterance by subsequence DTW under --qbe-distance, and the ranking is scored against the term tokens
of --qbe-item.  summary.json gains "qbe": {"z1": {map, p_at_n, p_at_10, located, no_target}, "feats": {...}, "queries", "dropped",
"distance", "frame_shift", "frame_offset"} (--qbe-on chooses; the frame grid is --abx-frame-shift / --abx-frame-offset).

With --baseline-feat-scp SCP [--baseline-name mfcc] a second Kaldi archive with the same keys and the same frame count per
utterance (MFCC + deltas + CMVN from prepare_kaldi_data.py --mfcc_conf, the baseline the zero-resource literature quotes) is
scored as one more entry "<name>" of the "abx", "units" and "qbe" blocks, with abx_by_pair_<name>.tsv, units_<name>.txt and
units_centroids_<name>.npy beside those of z1 and feats.  It is taken as it is (not normalised by --mvn-path); a key it lacks or
another frame count is an error that names the key.

With --probe-item FILE (needs --feat-scp data) a linear probe (probe.py: softmax regression, L-BFGS, --probe-l2, --probe-iters) is
trained on the frames of all but the last ceil(--probe-holdout U) utterances of RandomState(--probe-seed).permutation(U) to predict
each frame's phone and its speaker (--probe-target), on frame-level z1 and on the normalised input (--probe-on) and on the
--baseline-feat-scp archive, and scored on the held-out utterances.  summary.json gains "probe": {"phone": {"z1": {classes,
train_frames, test_frames, accuracy, balanced_accuracy, majority, train_accuracy, loss, iterations, converged, l2, unlabelled,
overlaps}, "feats": {...}}, "speaker": {...}, "holdout", "seed", "frame_shift", "frame_offset"} (the frame grid is
--abx-frame-shift / --abx-frame-offset).  Without --probe-item every output is what it was.

With --per-item FILE (needs --feat-scp data) phones are recognised (phonerec.py: the phone probe's scores, a Viterbi pass under a
frame-level phone bigram, the phone error rate against the alignment read in onset order) on the held-out utterances of the
probe's split (--probe-holdout, --probe-seed, --probe-l2, --probe-iters), on frame-level z1 and on the normalised input (--per-on)
and on the --baseline-feat-scp archive.  summary.json gains "per": {"z1": {per, sub, del, ins, cor, ref_tokens, utterances,
per_argmax, frame_accuracy, frame_accuracy_argmax, classes, ...}, "feats": {...}, "holdout", "seed", "frame_shift",
"frame_offset", "phone_penalty"}; --per-phone-map folds both sides, --per-phone-penalty is the insertion penalty.  Without
--per-item every output is what it was.  With --per-ctc every entry of --per-on gains "ctc": {per, sub, del, ins, cor, objective,
iterations, converged, context, dropped_infeasible, ...}: the same linear model trained by CTC (ctc.py) on the transcriptions of
the training utterances alone, decoded greedily; --per-ctc-context K splices K frames per side.  With --per-ctc-beam W
[--per-ctc-lm-scale S --per-ctc-bonus B | --per-ctc-lm-tune] [--per-ctc-class-beam G] [--per-ctc-lm-smooth A] every entry also gains
"ctc_beam" beside "ctc": the same model decoded by prefix beam search with a phone bigram (ctcbeam.py): the error rate's keys, beam,
lm_scale, bonus, class_beam, smooth and the tuning grid.

Real features (--feat-scp / --len-scp) are written un-normalised (NumpyDataset.undo_mvn); without them the data is the synthetic
split of train_model.py (its dev split for the same --seed).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Evaluate a trained (Simple)FHVAE checkpoint: latents, mu2, reconstructions, conversion")
    p.add_argument("--checkpoint", required=True)
    p.add_argument("--out", required=True, help="output directory (created)")
    p.add_argument("--data-format", default="numpy", choices=["numpy", "kaldi"],
                   help="what --feat-scp points at: .npy files or Kaldi archives (as train_model.py)")
    p.add_argument("--feat-scp", default=None)
    p.add_argument("--len-scp", default=None)
    p.add_argument("--min-len", type=int, default=None)
    p.add_argument("--mvn-path", default=None)
    p.add_argument("--seg-shift", type=int, default=8)
    # synthetic data (train_model.py's flags)
    p.add_argument("--seg-len", type=int, default=20)
    p.add_argument("--mels", type=int, default=80)
    p.add_argument("--num-seqs", type=int, default=100)
    p.add_argument("--segments", type=int, default=250)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--batch-size", type=int, default=2048)
    p.add_argument("--convert-to", type=int, default=None, help="sequence index whose mu2 replaces z2 of the reconstructed segments")
    p.add_argument("--max-recon", type=int, default=16)
    p.add_argument("--wav-out", default=None, help="directory for the synthesized WAV files (needs --feat-scp spec features)")
    p.add_argument("--wav-seqs", type=int, default=0, help="synthesize the first N sequences of the data")
    p.add_argument("--sr", type=int, default=16000, help="sample rate the features were taken at")
    p.add_argument("--win-t", type=float, default=0.025)
    p.add_argument("--hop-t", type=float, default=0.010)
    p.add_argument("--gl-iters", type=int, default=32, help="Griffin-Lim rounds")
    p.add_argument("--gl-seed", type=int, default=0, help="seed of the initial phases")
    p.add_argument("--wav-ftype", default="spec", choices=["spec", "fbank"],
                   help="feature type of the --feat-scp data for --wav-out; fbank: mel inversion in front of Griffin-Lim")
    p.add_argument("--nnls-iters", type=int, default=200, help="steps of the mel inversion (--wav-ftype fbank)")
    spk = p.add_mutually_exclusive_group()
    spk.add_argument("--utt2spk", default=None, help="speaker verification: Kaldi utt2spk file naming each sequence's speaker (needs --feat-scp)")
    spk.add_argument("--spk-key-sep", default=None,
                     help="speaker verification: the speaker is the sequence key up to the first SEP (needs --feat-scp)")
    p.add_argument("--sv-bins", type=int, default=4096, help="score bins of the verification histograms (a power of two, 64..8192)")
    p.add_argument("--sv-backend", nargs="+", default=None, choices=["cosine", "lda", "plda"],
                   help="speaker verification: besides the raw cosine, score after an LDA (lda) and by a PLDA log-likelihood ratio (plda) "
                        "trained on the sequences of --sv-train-feat-scp (spk_backend.py)")
    p.add_argument("--sv-train-feat-scp", default=None, metavar="SCP", help="--sv-backend lda / plda: the training sequences (same format as --feat-scp)")
    p.add_argument("--sv-train-len-scp", default=None, metavar="SCP")
    p.add_argument("--sv-lda-dim", type=int, default=None, metavar="K", help="columns the LDA keeps (needed by lda; plda alone: no LDA in front)")
    p.add_argument("--sv-plda-iters", type=int, default=10, metavar="N", help="EM iterations of the PLDA")
    p.add_argument("--sv-no-length-norm", action="store_true", help="no length normalisation between the LDA and the PLDA")
    p.add_argument("--sv-snorm", action="store_true", help="--sv-backend lda / plda: also the scores normalised against the training speakers' means")
    p.add_argument("--sv-snorm-top", type=int, default=200, metavar="K", help="cohort scores kept per side (0: the whole cohort)")
    p.add_argument("--tsne", action="store_true", help="write exact t-SNE maps of mu2 and of the sequences' mean z1 (needs --feat-scp)")
    p.add_argument("--tsne-perplexity", type=float, default=30.0, help="at most (sequences - 1) / 3")
    p.add_argument("--tsne-iters", type=int, default=1000)
    p.add_argument("--tsne-seed", type=int, default=0, help="seed of the initial map")
    p.add_argument("--abx-item", default=None, metavar="FILE", help="ABX phone discriminability of the tokens this .item file lists (needs --feat-scp)")
    p.add_argument("--abx-on", nargs="+", default=["z1", "feats"], choices=["z1", "feats"], help="what to score: frame-level z1, the input features")
    p.add_argument("--abx-distance", default="angular", choices=["angular", "cosine"], help="frame cost under the DTW")
    p.add_argument("--abx-frame-shift", type=float, default=0.010, help="seconds between frames")
    p.add_argument("--abx-frame-offset", type=float, default=0.0,
                   help="time of frame 0 in seconds (0.0125 for Kaldi snip-edges frames of 25 ms, whose centres lie half a window in)")
    p.add_argument("--abx-max-per-cell", type=int, default=20, help="tokens kept per (phone, context, speaker), the first in file order; 0: all")
    p.add_argument("--units", type=int, default=None, metavar="K", help="discrete units: a k-means codebook of K centroids, one unit per frame (needs --feat-scp)")
    p.add_argument("--units-on", nargs="+", default=["z1", "feats"], choices=["z1", "feats"], help="what to quantise: frame-level z1, the input features")
    p.add_argument("--units-iters", type=int, default=100, help="Lloyd iterations, at most")
    p.add_argument("--units-seed", type=int, default=0, help="seed of the rows the first centroids are copied from")
    p.add_argument("--units-item", default=None, metavar="FILE", help="phone alignment (.item) to score the units against")
    p.add_argument("--units-segment", action="store_true", help="with --units: segment every utterance over the codebook (segment.py)")
    p.add_argument("--units-dur-penalty", type=float, default=1.0, metavar="LAMBDA", help="--units-segment: the penalty per segment")
    p.add_argument("--units-max-seg-frames", type=int, default=32, metavar="L", help="--units-segment: frames per segment, at most (1 .. 64)")
    p.add_argument("--qbe-queries", default=None, metavar="ITEM",
                   help="query-by-example search: the examples (.item, the #phone column is the term) cut from and searched in --feat-scp data")
    p.add_argument("--qbe-item", default=None, metavar="ITEM", help="the term tokens of the corpus the search is scored against")
    p.add_argument("--qbe-on", nargs="+", default=["z1", "feats"], choices=["z1", "feats"], help="what to search on: frame-level z1, the input features")
    p.add_argument("--qbe-distance", default="angular", choices=["angular", "cosine"], help="frame cost under the subsequence DTW")
    p.add_argument("--qbe-max-per-term", type=int, default=5, help="queries kept per term, the first in file order; 0: all")
    p.add_argument("--baseline-feat-scp", default=None, metavar="SCP",
                   help="a second Kaldi archive (same keys, same frames per utterance) scored beside z1 and feats under --abx-item / --units / --qbe-queries")
    p.add_argument("--baseline-name", default=None, help="the baseline's entry in summary.json and its files' suffix (default mfcc)")
    p.add_argument("--probe-item", default=None, metavar="FILE",
                   help="frame probes: a softmax regression on the frames of --feat-scp data predicts the phone / speaker this .item alignment gives")
    p.add_argument("--probe-target", nargs="+", default=["phone", "speaker"], choices=["phone", "speaker"], help="what the probe predicts")
    p.add_argument("--probe-on", nargs="+", default=["z1", "feats"], choices=["z1", "feats"], help="what to probe: frame-level z1, the input features")
    p.add_argument("--probe-holdout", type=float, default=0.2, help="share of the utterances held out as the probe's test set")
    p.add_argument("--probe-seed", type=int, default=0, help="seed of the held-out utterances")
    p.add_argument("--probe-l2", type=float, default=1e-4)
    p.add_argument("--probe-iters", type=int, default=200, help="L-BFGS iterations, at most")
    p.add_argument("--per-item", default=None, metavar="FILE",
                   help="phone recognition: the phone error rate of a Viterbi pass over the phone probe's scores against this .item alignment")
    p.add_argument("--per-on", nargs="+", default=["z1", "feats"], choices=["z1", "feats"], help="what to recognise on: frame-level z1, the input features")
    p.add_argument("--per-phone-map", default=None, metavar="FILE", help="lines `phone target` (`-` deletes) applied to both sides")
    p.add_argument("--per-phone-penalty", type=float, default=0.0, help="subtracted from every transition between different phones")
    p.add_argument("--per-ctc", action="store_true", help="with --per-item: also train by CTC on the transcriptions alone, decode greedily")
    p.add_argument("--per-ctc-context", type=int, default=0, metavar="K", help="frames spliced per side for --per-ctc")
    p.add_argument("--per-ctc-beam", type=int, default=None, metavar="W", help="with --per-ctc: also decode by prefix beam search of this width with a phone bigram")
    p.add_argument("--per-ctc-lm-scale", type=float, default=None, metavar="S", help="the bigram's weight (default 1)")
    p.add_argument("--per-ctc-bonus", type=float, default=None, metavar="B", help="added per phone put out (default 0)")
    p.add_argument("--per-ctc-lm-tune", action="store_true", help="choose the weight and the bonus on the training utterances instead")
    p.add_argument("--per-ctc-class-beam", type=float, default=float("inf"), metavar="G", help="classes further than this below the frame's best are not extended into")
    p.add_argument("--per-ctc-lm-smooth", type=float, default=1.0, metavar="A", help="added to every bigram count")
    return p


def parse_args(argv=None) -> argparse.Namespace:
    p = build_parser()
    args = p.parse_args(argv)
    if (args.utt2spk is not None or args.spk_key_sep is not None) and args.feat_scp is None:
        p.error("--utt2spk / --spk-key-sep name the speakers of --feat-scp data: give --feat-scp")
    if args.sv_bins < 64 or args.sv_bins > 8192 or args.sv_bins & (args.sv_bins - 1):
        p.error("--sv-bins %d must be a power of two in [64, 8192]" % args.sv_bins)
    args.sv_trained = [b for b in ("lda", "plda") if b in (args.sv_backend or [])]
    if args.sv_trained:
        if args.utt2spk is None and args.spk_key_sep is None:
            p.error("--sv-backend scores the trials of --utt2spk / --spk-key-sep: give one of them")
        if args.sv_train_feat_scp is None or args.sv_train_len_scp is None:
            p.error("--sv-backend %s is trained on --sv-train-feat-scp / --sv-train-len-scp: give both" % " ".join(args.sv_trained))
        if "lda" in args.sv_trained and args.sv_lda_dim is None:
            p.error("--sv-backend lda needs --sv-lda-dim")
        if (args.sv_lda_dim is not None and args.sv_lda_dim < 1) or args.sv_plda_iters < 0:
            p.error("--sv-lda-dim must be at least 1 and --sv-plda-iters not negative")
        if args.sv_snorm_top < 0:
            p.error("--sv-snorm-top %d must not be negative" % args.sv_snorm_top)
    elif (args.sv_train_feat_scp is not None or args.sv_train_len_scp is not None or args.sv_lda_dim is not None or args.sv_plda_iters != 10
          or args.sv_no_length_norm):
        p.error("--sv-train-feat-scp, --sv-train-len-scp, --sv-lda-dim, --sv-plda-iters and --sv-no-length-norm need --sv-backend lda or plda")
    elif args.sv_snorm or args.sv_snorm_top != 200:
        p.error("--sv-snorm and --sv-snorm-top need --sv-backend lda or plda")
    if args.tsne and args.feat_scp is None:
        p.error("--tsne draws the sequences of --feat-scp data: give --feat-scp")
    if not args.tsne_perplexity >= 1.0:
        p.error("--tsne-perplexity %g must be at least 1" % args.tsne_perplexity)
    if args.tsne_iters < 1:
        p.error("--tsne-iters %d must be at least 1" % args.tsne_iters)
    if args.tsne_seed < 0 or args.tsne_seed >= 2 ** 32:
        p.error("--tsne-seed %d must lie in [0, 2^32)" % args.tsne_seed)
    if args.abx_item is not None and args.feat_scp is None:
        p.error("--abx-item lists tokens of --feat-scp data: give --feat-scp")
    if not args.abx_frame_shift > 0:
        p.error("--abx-frame-shift %g must be positive" % args.abx_frame_shift)
    if args.abx_max_per_cell < 0:
        p.error("--abx-max-per-cell %d must not be negative" % args.abx_max_per_cell)
    if args.units is not None and args.feat_scp is None:
        p.error("--units quantises the frames of --feat-scp data: give --feat-scp")
    if args.units is not None and args.units < 1:
        p.error("--units %d must be at least 1" % args.units)
    if args.units_segment and args.units is None:
        p.error("--units-segment segments over the codebook of --units: give --units K")
    if not args.units_dur_penalty >= 0 or not 1 <= args.units_max_seg_frames <= 64:
        p.error("--units-dur-penalty must be at least 0 and --units-max-seg-frames lie in [1, 64]")
    if args.units_iters < 1:
        p.error("--units-iters %d must be at least 1" % args.units_iters)
    if args.units_seed < 0 or args.units_seed >= 2 ** 32:
        p.error("--units-seed %d must lie in [0, 2^32)" % args.units_seed)
    if (args.qbe_queries is None) != (args.qbe_item is None):
        p.error("--qbe-queries and --qbe-item come together")
    if args.qbe_queries is not None and args.feat_scp is None:
        p.error("--qbe-queries lists tokens of --feat-scp data: give --feat-scp")
    if args.qbe_max_per_term < 0:
        p.error("--qbe-max-per-term %d must not be negative" % args.qbe_max_per_term)
    if args.probe_item is not None and args.feat_scp is None:
        p.error("--probe-item labels the frames of --feat-scp data: give --feat-scp")
    if not 0.0 < args.probe_holdout < 1.0:
        p.error("--probe-holdout %g must lie in (0, 1)" % args.probe_holdout)
    if args.probe_seed < 0 or args.probe_seed >= 2 ** 32:
        p.error("--probe-seed %d must lie in [0, 2^32)" % args.probe_seed)
    if args.probe_iters < 0 or not args.probe_l2 >= 0:
        p.error("--probe-iters and --probe-l2 must not be negative")
    if args.per_item is not None and args.feat_scp is None:
        p.error("--per-item transcribes the utterances of --feat-scp data: give --feat-scp")
    if args.per_ctc and args.per_item is None:
        p.error("--per-ctc needs --per-item")
    if args.per_ctc_context < 0 or (args.per_ctc_context != 0 and not args.per_ctc):
        p.error("--per-ctc-context must not be negative and needs --per-ctc")
    beam_flags = (args.per_ctc_lm_scale is not None or args.per_ctc_bonus is not None or args.per_ctc_lm_tune
                  or args.per_ctc_class_beam != float("inf") or args.per_ctc_lm_smooth != 1.0)
    if args.per_ctc_beam is None and beam_flags:
        p.error("--per-ctc-lm-scale, --per-ctc-bonus, --per-ctc-lm-tune, --per-ctc-class-beam and --per-ctc-lm-smooth need --per-ctc-beam")
    if args.per_ctc_beam is not None and (not args.per_ctc or not 1 <= args.per_ctc_beam <= 64):
        p.error("--per-ctc-beam needs --per-ctc and a width from 1 to 64")
    if args.per_ctc_lm_tune and (args.per_ctc_lm_scale is not None or args.per_ctc_bonus is not None):
        p.error("--per-ctc-lm-tune excludes --per-ctc-lm-scale and --per-ctc-bonus")
    if ((args.per_ctc_lm_scale is not None and not 0 <= args.per_ctc_lm_scale < float("inf"))
            or (args.per_ctc_bonus is not None and not np.isfinite(args.per_ctc_bonus))):
        p.error("--per-ctc-lm-scale must be finite and not negative, --per-ctc-bonus finite")
    if not args.per_ctc_class_beam >= 0 or not args.per_ctc_lm_smooth >= 0:
        p.error("--per-ctc-class-beam and --per-ctc-lm-smooth must not be negative")
    if not np.isfinite(args.per_phone_penalty):
        p.error("--per-phone-penalty must be finite")
    if args.baseline_name is not None and args.baseline_feat_scp is None:
        p.error("--baseline-name needs --baseline-feat-scp")
    if args.baseline_feat_scp is not None:
        if args.abx_item is None and args.units is None and args.qbe_queries is None and args.probe_item is None and args.per_item is None:
            p.error("--baseline-feat-scp is scored by --abx-item, --units and --qbe-queries: give one of them")
        args.baseline_name = "mfcc" if args.baseline_name is None else args.baseline_name
        if args.baseline_name in ("z1", "feats") or not args.baseline_name.replace("_", "").replace("-", "").isalnum():
            p.error("--baseline-name %r: letters, digits, - and _, and neither z1 nor feats" % args.baseline_name)
    return args


def speakers_of(args, keys):
    """--utt2spk / --spk-key-sep: the speaker of every key (None = unknown)."""
    import verification as V

    if args.utt2spk is not None:
        table = V.read_utt2spk(args.utt2spk)
        return [table.get(k) for k in keys]
    return V.speakers_from_keys(keys, args.spk_key_sep)


def sequence_means(z1_mu, seq_pos, n, dev):
    """z1_mu (segments, D) with seq_pos the row each segment belongs to -> (n, D) means on dev."""
    z1 = torch.from_numpy(z1_mu).to(dev)
    pos = torch.from_numpy(seq_pos).to(dev)
    z1_sum = torch.zeros(n, z1.shape[1], device=dev).index_add_(0, pos, z1)
    count = torch.zeros(n, device=dev).index_add_(0, pos, torch.ones(pos.shape[0], device=dev))
    return z1_sum / count.clamp(min=1.0).unsqueeze(1)


def sv_train_embeddings(args, model, T, dev):
    """--sv-train-feat-scp / --sv-train-len-scp: the training sequences through the model -> (keys, {"mu2": (n, D) numpy, "z1_mean":
    (n, D) numpy}), the embeddings verify_speakers scores, of the sequences the back end is trained on."""
    import utils
    from datasets import KaldiDataset, NumpyDataset, ResidentSegmentPool

    Dataset = NumpyDataset if args.data_format == "numpy" else KaldiDataset
    ds = Dataset(args.sv_train_feat_scp, args.sv_train_len_scp, args.min_len if args.min_len is not None else T, args.mvn_path, T,
                 args.seg_shift, False)
    pool = ResidentSegmentPool(ds, dev)
    z1s, ids = [], []
    with torch.no_grad():
        for idxs, x, _ in pool.epoch(args.batch_size, shuffle=False):
            z1s.append(model.encode(x)[0].cpu().numpy()), ids.append(torch.as_tensor(idxs).cpu().numpy())
        mu2 = utils.estimate_mu2_dict(model, pool.epoch(args.batch_size, shuffle=False), len(ds))
    seqs = sorted(mu2)
    if not seqs:
        raise ValueError("%s holds no sequence long enough" % args.sv_train_feat_scp)
    seq_pos = np.searchsorted(np.asarray(seqs, dtype=np.int64), np.concatenate(ids).astype(np.int64))
    z1_mean = sequence_means(np.concatenate(z1s), seq_pos, len(seqs), dev).cpu().numpy()
    return [ds.seq_keys[y] for y in seqs], {"mu2": np.stack([mu2[y].cpu().numpy() for y in seqs]), "z1_mean": z1_mean}


def verify_speakers(args, keys, mu2_rows, z1_mu, seq_pos, out_dir, dev, train=None):
    """--utt2spk / --spk-key-sep: the "speaker_verification" block of summary.json (see the module docstring).  keys: the key of
    every row of mu2_rows; z1_mu (segments, D) with seq_pos the row each segment belongs to.  train: sv_train_embeddings' pair
    for --sv-backend lda / plda: every embedding's entry gains "lda" / "plda" (spk_backend.Backend.score_all_pairs' figures), and
    sv_hist_<name>_<backend>.npy and sv_backend_<name>.npz are written."""
    import verification as V

    labels, n_spk = V.labels_from_speakers(speakers_of(args, keys))
    z1_mean = sequence_means(z1_mu, seq_pos, len(keys), dev)
    block = {}
    for name, emb in (("mu2", torch.from_numpy(mu2_rows).to(dev)), ("z1_mean", z1_mean)):
        r = V.speaker_verification(emb, labels, n_bins=args.sv_bins, device=dev)
        np.save(os.path.join(out_dir, "sv_hist_%s.npy" % name), r.pop("hist"))
        block[name] = r
        if train is not None:
            import spk_backend as SB

            train_labels, _ = V.labels_from_speakers(speakers_of(args, train[0]))
            backend = SB.fit(train[1][name], train_labels, args.sv_lda_dim, not args.sv_no_length_norm, args.sv_plda_iters)
            for b in args.sv_trained:
                rb = backend.score_all_pairs(emb, labels, n_bins=args.sv_bins, backend=b, device=dev)
                np.save(os.path.join(out_dir, "sv_hist_%s_%s.npy" % (name, b)), rb.pop("hist"))
                if args.sv_snorm:
                    import score_norm as SN

                    cohort = SN.make_cohort(train[1][name], train_labels, "speaker-means")
                    rn = SN.score_all_pairs(backend, emb, labels, cohort, top=args.sv_snorm_top, which=b, n_bins=args.sv_bins, device=dev)
                    np.save(os.path.join(out_dir, "sv_hist_%s_%s_snorm.npy" % (name, b)), rn.pop("hist"))
                    rb["snorm"] = rn
                r[b] = rb
            backend.save(os.path.join(out_dir, "sv_backend_%s.npz" % name))
    block.update({"speakers": n_spk, "unlabelled": int((labels < 0).sum()), "bins": args.sv_bins})
    return block


def draw_tsne(args, keys, mu2_rows, z1_mu, seq_pos, out_dir, dev):
    """--tsne: the maps, tsne.tsv, the pictures and the "tsne" block of summary.json (see the module docstring)."""
    import tsne as T
    import verification as V

    known = args.utt2spk is not None or args.spk_key_sep is not None
    speakers = speakers_of(args, keys) if known else [None] * len(keys)
    labels, _ = V.labels_from_speakers(speakers)
    block = {"perplexity": args.tsne_perplexity, "iterations": args.tsne_iters, "seed": args.tsne_seed}
    maps = {}
    for name, emb in (("mu2", torch.from_numpy(mu2_rows).to(dev)), ("z1_mean", sequence_means(z1_mu, seq_pos, len(keys), dev))):
        maps[name], info = T.tsne(emb, perplexity=args.tsne_perplexity, n_iter=args.tsne_iters, seed=args.tsne_seed, device=dev)
        np.save(os.path.join(out_dir, "tsne_%s.npy" % name), maps[name])
        block["kl_%s" % name] = info["kl"]
    with open(os.path.join(out_dir, "tsne.tsv"), "w") as f:
        for k, spk, a, b in zip(keys, speakers, maps["mu2"], maps["z1_mean"]):
            f.write("%s\t%s\t%.6g\t%.6g\t%.6g\t%.6g\n" % (k, "-" if spk is None else spk, a[0], a[1], b[0], b[1]))
    if known:
        for name in maps:
            if not T.scatter_png(os.path.join(out_dir, "tsne_%s.png" % name), maps[name], labels, "t-SNE of %s by speaker" % name):
                print("--tsne: matplotlib is not installed, no tsne_*.png (the maps are in tsne_*.npy and tsne.tsv)")
                break
    return block


def baseline_rows(args, pool, dev):
    """--baseline-feat-scp: the archive's matrices in the order of the pool's utterances, stacked on the device -> (frames, D)
    f32.  A key the archive lacks, or a matrix whose row count is not the utterance's frame count, raises ValueError naming it."""
    import kaldi_io_lite

    specs = {}
    with open(args.baseline_feat_scp) as fh:
        for ln, line in enumerate(fh, 1):
            parts = line.rstrip().split(None, 1)
            if not parts:
                continue
            if len(parts) != 2:
                raise ValueError("%s:%d: expected \"<key> <archive:offset>\"" % (args.baseline_feat_scp, ln))
            specs[parts[0]] = parts[1]
    mats = []
    for key, n in zip(pool.keys, pool.lengths):
        if key not in specs:
            raise ValueError("%s has no entry for %s" % (args.baseline_feat_scp, key))
        m = np.asarray(kaldi_io_lite.load_mat(specs[key]), dtype=np.float32)
        if m.ndim != 2 or len(m) != int(n) or (mats and m.shape[1] != mats[0].shape[1]):
            raise ValueError("%s: %s in %s, but %d frames in %s%s" % (key, "x".join(str(d) for d in m.shape), args.baseline_feat_scp, int(n), args.feat_scp,
                                                                     "" if not mats else " and %d columns before" % mats[0].shape[1]))
        mats.append(m)
    return torch.from_numpy(np.concatenate(mats, axis=0)).to(dev)


def measure_abx(args, model, T, out_dir, dev):
    """--abx-item: abx_by_pair_<on>.tsv and the "abx" block of summary.json (see the module docstring)."""
    import abx
    import frames

    pool = frames.pool_from_scp(args.data_format, args.feat_scp, args.len_scp, args.mvn_path, T, 1, dev)
    tokens = abx.tokens_from_items(abx.read_items(args.abx_item), pool.keys, pool.lengths, args.abx_frame_shift, args.abx_frame_offset,
                                   max_per_cell=args.abx_max_per_cell)
    block = {}
    ons = list(dict.fromkeys(args.abx_on)) + ([args.baseline_name] if args.baseline_feat_scp is not None else [])
    for on in ons:
        rows = baseline_rows(args, pool, dev) if on == args.baseline_name else frames.corpus_rows(model, pool, on, "ABX", args.batch_size)
        if rows.shape[1] > abx.ABX_MAX_DIM:
            raise ValueError("%s has %d values per frame, the DTW kernel takes at most %d" % (on, rows.shape[1], abx.ABX_MAX_DIM))
        res = abx.evaluate(rows.contiguous(), tokens, args.abx_distance)
        abx.write_by_pair(os.path.join(out_dir, "abx_by_pair_%s.tsv" % on), res, tokens["phones"])
        block[on] = {k: (None if isinstance(res[k], float) and np.isnan(res[k]) else res[k])
                     for k in ("within", "across", "cells_within", "cells_across", "triples_within", "triples_across")}
        del rows
    block.update({"tokens": int(tokens["start"].shape[0]), "dropped": tokens["dropped"], "distance": args.abx_distance,
                  "frame_shift": args.abx_frame_shift, "frame_offset": args.abx_frame_offset})
    return block


def search_terms(args, model, T, out_dir, dev):
    """--qbe-queries: the "qbe" block of summary.json (see the module docstring)."""
    import abx
    import frames
    import qbe

    pool = frames.pool_from_scp(args.data_format, args.feat_scp, args.len_scp, args.mvn_path, T, 1, dev)
    queries = qbe.queries_from_items(abx.read_items(args.qbe_queries), pool.keys, pool.lengths, args.abx_frame_shift, args.abx_frame_offset,
                                     max_per_term=args.qbe_max_per_term)
    truth = qbe.truth_from_items(abx.read_items(args.qbe_item), pool.keys, pool.lengths, args.abx_frame_shift, args.abx_frame_offset)
    block = {}
    ons = list(dict.fromkeys(args.qbe_on)) + ([args.baseline_name] if args.baseline_feat_scp is not None else [])
    for on in ons:
        rows = qbe.checked_rows(baseline_rows(args, pool, dev), on) if on == args.baseline_name else qbe.corpus_rows(model, pool, on, args.batch_size)
        res, _ = qbe.evaluate(rows, queries, rows, qbe.utt_ptr_of(pool.lengths), truth, args.qbe_distance)
        block[on] = {k: res[k] for k in ("map", "p_at_n", "p_at_10", "located", "no_target")}
        del rows
    block.update({"queries": len(queries["id"]), "dropped": queries["dropped"], "distance": args.qbe_distance,
                  "frame_shift": args.abx_frame_shift, "frame_offset": args.abx_frame_offset})
    return block


def discover_units(args, model, T, out_dir, dev):
    """--units: units_<on>.txt, units_centroids_<on>.npy and the "units" block of summary.json (see the module docstring)."""
    import abx
    import frames
    import units

    pool = frames.pool_from_scp(args.data_format, args.feat_scp, args.len_scp, args.mvn_path, T, 1, dev)
    items = abx.read_items(args.units_item) if args.units_item is not None else None
    block = {}
    ons = list(dict.fromkeys(args.units_on)) + ([args.baseline_name] if args.baseline_feat_scp is not None else [])
    for on in ons:
        if on == args.baseline_name:
            rows = baseline_rows(args, pool, dev)
            width = int(rows.shape[1])
            if width > units.KM_MAX_DIM:
                raise ValueError("%s has %d values per frame, the k-means kernels take at most %d" % (on, width, units.KM_MAX_DIM))
            rows = torch.nn.functional.pad(rows, (0, -width % 16)).contiguous()  # (as units.corpus_rows pads z1 and feats)
        else:
            rows, width = units.corpus_rows(model, pool, on, args.batch_size)
        info, cent, _, seqs = units.discover(rows, width, pool.keys, pool.lengths, on, k=args.units, iters=args.units_iters,
                                             seed=args.units_seed, items=items, frame_shift=args.abx_frame_shift,
                                             frame_offset=args.abx_frame_offset)
        np.save(os.path.join(out_dir, "units_centroids_%s.npy" % on), cent)
        units.write_units(os.path.join(out_dir, "units_%s.txt" % on), pool.keys, seqs)
        if args.units_segment:
            import segment

            info["segments"], segs, seg_items = segment.discover(rows, cent, pool.keys, pool.lengths, args.units_dur_penalty,
                                                                 args.units_max_seg_frames, info["k"], items=items,
                                                                 frame_shift=args.abx_frame_shift, frame_offset=args.abx_frame_offset)
            abx.write_items(os.path.join(out_dir, "segments_%s.item" % on), seg_items)
            units.write_units(os.path.join(out_dir, "segments_%s.txt" % on), pool.keys, [un for _, un in segs])
        block[on] = info
        del rows
    return block


def probe_frames(args, model, T, out_dir, dev):
    """--probe-item: the "probe" block of summary.json (see the module docstring)."""
    import abx
    import frames
    import probe
    from fit_gmm import corpus_rows
    from probe_latents import split_rows

    pool = frames.pool_from_scp(args.data_format, args.feat_scp, args.len_scp, args.mvn_path, T, 1, dev)
    items = abx.read_items(args.probe_item)
    block = {}
    ons = list(dict.fromkeys(args.probe_on)) + ([args.baseline_name] if args.baseline_feat_scp is not None else [])
    for target in dict.fromkeys(args.probe_target):
        labels, names, overlaps = probe.frame_labels(items, pool.keys, pool.lengths, target, args.abx_frame_shift, args.abx_frame_offset)
        if not names:
            raise ValueError("no frame lies under a token of %s" % args.probe_item)
        block[target] = {}
        for on in ons:
            rows = baseline_rows(args, pool, dev) if on == args.baseline_name else corpus_rows(model, pool, on, args.batch_size)
            if rows.shape[1] > probe.PROBE_MAX_W:
                raise ValueError("%s has %d values per frame, the probe kernels take at most %d" % (on, rows.shape[1], probe.PROBE_MAX_W))
            split = split_rows(rows.contiguous(), labels, pool.lengths, args.probe_holdout, args.probe_seed)
            _, report, _ = probe.run(*split, names, l2=args.probe_l2, iters=args.probe_iters)
            report.update({"unlabelled": int((labels < 0).sum()), "overlaps": int(overlaps)})
            block[target][on] = report
            del rows
    block.update({"holdout": args.probe_holdout, "seed": args.probe_seed, "frame_shift": args.abx_frame_shift,
                  "frame_offset": args.abx_frame_offset})
    return block


def per_phones(args, model, T, dev):
    """--per-item: the "per" block of summary.json (see the module docstring)."""
    import abx
    import frames
    import phonerec
    import probe
    from fit_gmm import corpus_rows
    from recognise_phones import reference_ids, split_corpus

    pool = frames.pool_from_scp(args.data_format, args.feat_scp, args.len_scp, args.mvn_path, T, 1, dev)
    items = abx.read_items(args.per_item)
    labels, names, _ = probe.frame_labels(items, pool.keys, pool.lengths, "phone", args.abx_frame_shift, args.abx_frame_offset)
    if not names:
        raise ValueError("no frame lies under a token of %s" % args.per_item)
    refs = reference_ids(phonerec.references(items, pool.keys), names)
    table = phonerec.read_phone_map(args.per_phone_map, names)[0] if args.per_phone_map is not None else None
    block = {}
    for on in list(dict.fromkeys(args.per_on)) + ([args.baseline_name] if args.baseline_feat_scp is not None else []):
        rows = baseline_rows(args, pool, dev) if on == args.baseline_name else corpus_rows(model, pool, on, args.batch_size)
        if rows.shape[1] > probe.PROBE_MAX_W:
            raise ValueError("%s has %d values per frame, the probe kernels take at most %d" % (on, rows.shape[1], probe.PROBE_MAX_W))
        train, test = split_corpus(rows.contiguous(), labels, pool.lengths, refs, pool.keys, args.probe_holdout, args.probe_seed)
        block[on] = phonerec.recognise(train[0], train[1], train[2], test[0], test[2], test[3], names, l2=args.probe_l2, iters=args.probe_iters,
                                       penalty=args.per_phone_penalty, phone_table=table, test_y=test[1])[1]
        if args.per_ctc:
            import ctc

            train_refs = [refs[u] for u in probe.split_utterances(len(pool.lengths), args.probe_holdout, args.probe_seed)[0]]
            ctc_out = ctc.recognise(train[0], train[2], train_refs, test[0], test[2], test[3], names, l2=args.probe_l2,
                                    iters=args.probe_iters, context=args.per_ctc_context, phone_table=table)
            block[on]["ctc"] = ctc_out[1]
            if args.per_ctc_beam is not None:
                import ctcbeam

                tuned = args.per_ctc_lm_tune
                block[on]["ctc_beam"] = ctcbeam.recognise(
                    train[0], train[2], train_refs, test[0], test[2], test[3], names, beam=args.per_ctc_beam,
                    scale=None if tuned else (1.0 if args.per_ctc_lm_scale is None else args.per_ctc_lm_scale),
                    bonus=None if tuned else (0.0 if args.per_ctc_bonus is None else args.per_ctc_bonus),
                    class_beam=args.per_ctc_class_beam, smooth=args.per_ctc_lm_smooth, phone_table=table, model=ctc_out[0])[1]
        del rows
    block.update({"holdout": args.probe_holdout, "seed": args.probe_seed, "frame_shift": args.abx_frame_shift,
                  "frame_offset": args.abx_frame_offset, "phone_penalty": args.per_phone_penalty})
    return block


def feature_width(model, seg_len):
    """Features per frame the checkpoint was trained on."""
    if hasattr(model, "n_feat"):
        return int(model.n_feat)
    return int(model.dec_gauss_layer.mulayer.out_features) // int(seg_len)  # (SimpleFHVAE works on flattened segments)


def write_wavs(args, model, ds, mu2, dev):
    """--wav-out: returns the list of files written (see the module docstring)."""
    import features
    import utils

    T, shift = ds.seg_len, ds.seg_shift
    os.makedirs(args.wav_out, exist_ok=True)
    names, specs = [], []
    with torch.no_grad():
        for si in range(min(args.wav_seqs, len(ds))):
            seq = ds.seq_keys[si]
            feat = np.load(ds.seq_feats[si]).astype(np.float32)
            nseg = (len(feat) - T) // shift + 1
            if nseg < 1:
                continue
            x = np.stack([ds.apply_mvn(feat[k * shift:k * shift + T]) for k in range(nseg)]).astype(np.float32)
            xd = torch.from_numpy(x).to(dev)
            decoded = [("recon", model.reconstruct(xd)[0])]
            if args.convert_to is not None:
                decoded.append(("to_%d" % args.convert_to, model.convert(xd, mu2[args.convert_to])[0]))
            covered = min(len(feat), (nseg - 1) * shift + T)
            names.append("%s_orig" % seq), specs.append(feat[:covered])
            for tag, mu in decoded:
                full, n = utils.overlap_mean(torch.from_numpy(np.asarray(ds.undo_mvn(mu.float().cpu().numpy()), dtype=np.float32)),
                                             T, shift, len(feat))
                assert n == covered
                names.append("%s_%s" % (seq, tag)), specs.append(full.numpy())
    if args.wav_ftype == "fbank":
        waves = features.synthesize_mel(specs, args.sr, args.win_t, args.hop_t, nnls_iters=args.nnls_iters, n_iter=args.gl_iters,
                                        seed=args.gl_seed, device=dev, names=names)
    else:
        waves = features.synthesize(specs, args.sr, args.win_t, args.hop_t, n_iter=args.gl_iters, seed=args.gl_seed, device=dev,
                                    names=names)
    files = []
    for name, y in zip(names, waves):
        features.write_wav(os.path.join(args.wav_out, name + ".wav"), y, args.sr)
        files.append(name + ".wav")
    return files


def main(argv=None) -> int:
    args = parse_args(argv)
    if args.wav_out is not None:
        import features

        if args.feat_scp is None:
            print("--wav-out needs --feat-scp data (\"spec\" features)", file=sys.stderr)
            return 1
        if args.data_format == "kaldi":
            print("--wav-out: Kaldi fbank features are not the features the synthesis inverts (use --data-format numpy data)",
                  file=sys.stderr)
            return 1
        try:
            n_fft, _ = features.check_synth_params(args.sr, args.win_t, args.hop_t, args.gl_iters, 0.99, 0.97)
            if args.wav_ftype == "fbank" and args.nnls_iters < 1:
                raise ValueError("--nnls-iters %d must be at least 1" % args.nnls_iters)
        except ValueError as e:
            print("--wav-out: %s" % e, file=sys.stderr)
            return 1
    if not torch.cuda.is_available():
        print("evaluation runs on a MI355X only (no CPU fallback)", file=sys.stderr)
        return 1
    import hip_binding as hb
    import utils
    from train_model import synthetic_split

    dev = torch.device("cuda:0")
    model = utils.load_checkpoint_file(args.checkpoint, finetune=True)[0].to(dev).eval()
    T = getattr(model, "seg_len", args.seg_len)
    undo = lambda a: a  # noqa: E731
    if args.feat_scp is not None:
        from datasets import KaldiDataset, NumpyDataset, ResidentSegmentPool

        Dataset = NumpyDataset if args.data_format == "numpy" else KaldiDataset
        ds = Dataset(args.feat_scp, args.len_scp, args.min_len if args.min_len is not None else T, args.mvn_path, T,
                     args.seg_shift, False)
        if args.wav_out is not None:
            cols = np.load(ds.seq_feats[0], mmap_mode="r").shape[1] if len(ds) else -1
            if args.wav_ftype == "fbank":
                width = feature_width(model, T)
                try:
                    if cols != width:
                        raise ValueError("the features have %d columns, but the checkpoint was trained on %d" % (cols, width))
                    features.check_melinv_params(args.sr, args.win_t, args.hop_t, cols, args.nnls_iters)
                except ValueError as e:
                    print("--wav-out --wav-ftype fbank: %s" % e, file=sys.stderr)
                    return 1
            elif cols != n_fft // 2 + 1:
                print("--wav-out: the features have %d columns, but --sr %d / --win-t %g need \"spec\" features of n_fft // 2 + 1 = %d "
                      "columns (mel \"fbank\" features cannot be inverted)" % (cols, args.sr, args.win_t, n_fft // 2 + 1), file=sys.stderr)
                return 1
        pool = ResidentSegmentPool(ds, dev)
        S = len(ds)
        undo = ds.undo_mvn

        def batches():
            return pool.epoch(args.batch_size, shuffle=False)
    else:
        S = args.num_seqs
        x_all, i_all, n_all = synthetic_split(args.segments, T, args.mels, S, args.seed + 2)
        x_all = x_all.to(dev)

        def batches():
            for s0 in range(0, x_all.shape[0], args.batch_size):
                yield i_all[s0:s0 + args.batch_size], x_all[s0:s0 + args.batch_size], n_all[s0:s0 + args.batch_size]

    hs_K = torch.load(args.checkpoint, map_location="cpu", weights_only=False).get("hierarchical_sequences")
    mu2_inject = None
    if hs_K is not None:
        # hierarchical sampling: the table holds the last training block's K sequences, not these.  S comes from the data, and
        # the lower bound is taken at each sequence's closed-form mu2 (estimated by the sorted, deterministic path; injected)
        from datasets import SyntheticSegmentPool
        from hierarchical import estimate_pool_mu2

        hs_pool = pool if args.feat_scp is not None else SyntheticSegmentPool(x_all, i_all, n_all, S, dev)
        mu2_inject = estimate_pool_mu2(model, hs_pool)
    elif model.mu2_table is not None:
        S = model.mu2_table.shape[0]
    z1s, z2s, ids, lbs, frames = [], [], [], [], 0
    recon_x = []
    with torch.no_grad():
        for idxs, x, nsegs in batches():
            z1, z2 = model.encode(x)
            z1s.append(z1.cpu().numpy()), z2s.append(z2.cpu().numpy()), ids.append(torch.as_tensor(idxs).cpu().numpy())
            zero = (torch.zeros(x.shape[0], model.z2_dim, device=dev), torch.zeros(x.shape[0], model.z1_dim, device=dev))
            lb = model(x, idxs, S, nsegs, eps=zero, mu2_table=mu2_inject)[0]
            lbs.append(float(lb.double().sum()))
            frames += x.shape[0] * x.shape[1]
            if sum(r.shape[0] for r in recon_x) < args.max_recon:
                recon_x.append(x[: args.max_recon - sum(r.shape[0] for r in recon_x)])
        mu2 = utils.estimate_mu2_dict(model, batches(), S)
        os.makedirs(args.out, exist_ok=True)
        out = lambda name, a: np.save(os.path.join(args.out, name), a)  # noqa: E731
        out("z1_mu.npy", np.concatenate(z1s)), out("z2_mu.npy", np.concatenate(z2s)), out("seq_ids.npy", np.concatenate(ids))
        seqs = sorted(mu2)
        out("mu2_seqs.npy", np.asarray(seqs, dtype=np.int64))
        mu2_rows = np.stack([mu2[y].cpu().numpy() for y in seqs]) if seqs else np.zeros((0, model.z2_dim), np.float32)
        out("mu2.npy", mu2_rows)
        if recon_x and args.max_recon > 0:
            xr = torch.cat(recon_x)
            x_mu, x_lv = model.reconstruct(xr)
            out("recon_x.npy", undo(xr.cpu().numpy())), out("recon_mu.npy", undo(x_mu.cpu().numpy()))
            out("recon_logvar.npy", x_lv.cpu().numpy())  # (in the normalised feature space)
            if args.convert_to is not None:
                if args.convert_to not in mu2:
                    print("--convert-to %d: no segment of that sequence in the data" % args.convert_to, file=sys.stderr)
                    return 1
                c_mu, c_lv = model.convert(xr, mu2[args.convert_to])
                out("convert_mu.npy", undo(c_mu.cpu().numpy())), out("convert_logvar.npy", c_lv.cpu().numpy())
    sv = None
    if args.utt2spk is not None or args.spk_key_sep is not None:
        seq_pos = np.searchsorted(np.asarray(seqs, dtype=np.int64), np.concatenate(ids).astype(np.int64))  # (mu2 covers every segment's sequence)
        try:
            train = sv_train_embeddings(args, model, T, dev) if args.sv_trained else None
            sv = verify_speakers(args, [ds.seq_keys[y] for y in seqs], mu2_rows, np.concatenate(z1s), seq_pos, args.out, dev, train)
        except (ValueError, OSError) as e:
            print("speaker verification: %s" % e, file=sys.stderr)
            return 1
    tsne_block = None
    if args.tsne:
        seq_pos = np.searchsorted(np.asarray(seqs, dtype=np.int64), np.concatenate(ids).astype(np.int64))
        try:
            tsne_block = draw_tsne(args, [ds.seq_keys[y] for y in seqs], mu2_rows, np.concatenate(z1s), seq_pos, args.out, dev)
        except (ValueError, OSError) as e:
            print("--tsne: %s" % e, file=sys.stderr)
            return 1
    abx_block = None
    if args.abx_item is not None:
        try:
            abx_block = measure_abx(args, model, T, args.out, dev)
        except (ValueError, OSError) as e:
            print("--abx-item: %s" % e, file=sys.stderr)
            return 1
    units_block = None
    if args.units is not None:
        try:
            units_block = discover_units(args, model, T, args.out, dev)
        except (ValueError, OSError) as e:
            print("--units: %s" % e, file=sys.stderr)
            return 1
    qbe_block = None
    if args.qbe_queries is not None:
        try:
            qbe_block = search_terms(args, model, T, args.out, dev)
        except (ValueError, OSError) as e:
            print("--qbe-queries: %s" % e, file=sys.stderr)
            return 1
    probe_block = None
    if args.probe_item is not None:
        try:
            probe_block = probe_frames(args, model, T, args.out, dev)
        except (ValueError, OSError) as e:
            print("--probe-item: %s" % e, file=sys.stderr)
            return 1
    per_block = None
    if args.per_item is not None:
        try:
            per_block = per_phones(args, model, T, dev)
        except (ValueError, OSError, RuntimeError) as e:
            print("--per-item: %s" % e, file=sys.stderr)
            return 1
    wavs = None
    if args.wav_out is not None:
        if args.convert_to is not None and args.convert_to not in mu2:
            print("--convert-to %d: no segment of that sequence in the data" % args.convert_to, file=sys.stderr)
            return 1
        wavs = write_wavs(args, model, ds, mu2, dev)
    if hb.lstm_sync_status() != 0:
        print("a persistent recurrence launch gave up: the results are invalid", file=sys.stderr)
        return 3
    summary = {"checkpoint": os.path.basename(args.checkpoint), "segments": int(sum(z.shape[0] for z in z1s)),
               "sequences": len(mu2), "lower_bound_per_frame": sum(lbs) / max(frames, 1)}
    if wavs is not None:
        summary["wavs"] = wavs
    if sv is not None:
        summary["speaker_verification"] = sv
    if tsne_block is not None:
        summary["tsne"] = tsne_block
    if abx_block is not None:
        summary["abx"] = abx_block
    if units_block is not None:
        summary["units"] = units_block
    if qbe_block is not None:
        summary["qbe"] = qbe_block
    if probe_block is not None:
        summary["probe"] = probe_block
    if per_block is not None:
        summary["per"] = per_block
    with open(os.path.join(args.out, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps(summary))
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main())
