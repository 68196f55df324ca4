"""fit_gmm.py -- soft acoustic units for a whole corpus: a diagonal-covariance Gaussian mixture on the frame-level z1 of a trained
checkpoint, or on the input features (the GMM-posteriorgram baseline of the zero-resource literature, on MFCC + deltas + CMVN
from prepare_kaldi_data.py --mfcc_conf), and the per-frame posteriors over its components (gmm.py does the work).

    python pytorch-scalablefhvae_amd/fit_gmm.py [--checkpoint CK] --feat-scp S --len-scp S [--data-format numpy|kaldi]
        [--mvn-path P] --out DIR (--k K | --model FILE.npz) [--on z1|feats] [--iters 50] [--tol 1e-4] [--seed 0]
        [--var-floor 0.01] [--kmeans-iters 10] [--batch-size B] [--compute-dtype f32|bf16]
        [--post-out DIR [--out-format kaldi|numpy]] [--item FILE [--frame-shift 0.010] [--frame-offset 0.0]]

  --checkpoint CK  optional.  Without it only --on feats is allowed: the archive's rows as read (normalised by --mvn-path if given)
  --k K            fit K components on this corpus (gmm.fit: EM from a k-means start drawn with --seed)
  --model FILE     apply a mixture fitted elsewhere (gmm.npz of another run); the width must match.  On the corpus it was fitted
                   on it reproduces that run's posteriorgrams and units.txt byte for byte
  --on z1          frames.encode_frames at shift 1: row f is frame f.  --on feats: the normalised input.  At most 64 values per
                   frame; a width that is no multiple of 8 is zero-padded on the device
  --post-out DIR   the (frames, K) posteriorgram of every utterance of --feat-scp, in order and none dropped, as an archive with
                   feats.scp / len.scp (extract_latents.write_archive).  eval_model.py --baseline-feat-scp DIR/feats.scp
                   --baseline-name gmm scores it under --abx-item, --units and --qbe-queries (those take widths up to 128)
  --item FILE      a phone alignment (abx.read_items): cluster purity, phone purity and PNMI of the arg-max components

It writes under --out: gmm.npz (weights, means, variances; float64), units.txt and units_collapsed.txt of the arg-max components
(units.write_units) and gmm.json: on, k, width, frames, iterations, converged, mean_loglik (per iteration), starved, floored,
seed and, with --item, cluster_purity, phone_purity, pnmi, labelled_frames, overlaps, phones, bitrate and bitrate_collapsed.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

POST_MAX_SCORED = 128  # (the widths eval_model.py's ABX and QbE take)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Soft acoustic units: a diagonal-covariance GMM and its posteriorgrams, on the GPU")
    p.add_argument("--checkpoint", default=None, help="optional: without it only --on feats")
    p.add_argument("--feat-scp", required=True)
    p.add_argument("--len-scp", required=True)
    p.add_argument("--data-format", default="numpy", choices=["numpy", "kaldi"], help="what --feat-scp points at")
    p.add_argument("--mvn-path", default=None)
    p.add_argument("--out", required=True, help="output directory (created)")
    how = p.add_mutually_exclusive_group(required=True)
    how.add_argument("--k", type=int, default=None, help="fit this many components on the corpus")
    how.add_argument("--model", default=None, metavar="FILE.npz", help="apply this mixture instead of fitting one")
    p.add_argument("--on", default="z1", choices=["z1", "feats"], help="frame-level z1, or the normalised input features")
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--tol", type=float, default=1e-4, help="stop when the mean log-likelihood rises by less than this share")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--var-floor", type=float, default=0.01, help="a variance is at least this share of the column's global variance")
    p.add_argument("--kmeans-iters", type=int, default=10, help="Lloyd iterations of the start")
    p.add_argument("--batch-size", type=int, default=16384, help="windows per forward")
    p.add_argument("--compute-dtype", default=None, choices=["f32", "bf16"], help="default: the checkpoint's")
    p.add_argument("--post-out", default=None, metavar="DIR", help="write every utterance's posteriorgram here")
    p.add_argument("--out-format", default="kaldi", choices=["kaldi", "numpy"], help="of --post-out")
    p.add_argument("--item", default=None, metavar="FILE", help="phone alignment to score the arg-max components against")
    p.add_argument("--frame-shift", type=float, default=0.010, help="seconds between frames")
    p.add_argument("--frame-offset", type=float, default=0.0, help="time of frame 0 in seconds")
    return p


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if args.checkpoint is None and args.on != "feats":
        p.error("--on %s needs --checkpoint: without --checkpoint only --on feats is possible" % args.on)
    if args.k is not None and args.k < 1:
        p.error("--k %d must be at least 1" % args.k)
    if args.iters < 1 or args.kmeans_iters < 1 or args.batch_size < 1:
        p.error("--iters, --kmeans-iters and --batch-size must be at least 1")
    if args.seed < 0 or args.seed >= 2 ** 32:
        p.error("--seed %d must lie in [0, 2^32)" % args.seed)
    if not args.var_floor > 0:
        p.error("--var-floor %g must be positive" % args.var_floor)
    if not args.frame_shift > 0:
        p.error("--frame-shift %g must be positive" % args.frame_shift)
    if args.compute_dtype is not None and args.checkpoint is None:
        p.error("--compute-dtype needs --checkpoint")
    return p, args


def corpus_rows(model, pool, on, batch_size):
    """The (total frames, width) f32 rows the mixture is fitted on: "z1", frames.encode_frames' frame-level z1; "feats", the
    normalised input."""
    import frames

    return frames.corpus_rows(model, pool, on, "the mixture", batch_size).contiguous()


def main(argv=None) -> int:
    parser, args = parse_args(argv)
    import torch

    model, T = None, 20
    if args.checkpoint is not None:
        import utils

        model = utils.load_checkpoint_file(args.checkpoint, finetune=True)[0].eval()
        T = int(getattr(model, "seg_len", 20))
        if args.compute_dtype is not None:
            if not hasattr(model, "compute_dtype"):
                parser.error("--compute-dtype: a %s checkpoint computes in f32 only" % model.model)
            model.compute_dtype = args.compute_dtype
    if not torch.cuda.is_available():
        print("the mixture runs on a MI355X only (no CPU fallback)", file=sys.stderr)
        return 1
    import abx
    import extract_latents
    import frames
    import gmm
    import hip_binding as hb
    import units

    dev = torch.device("cuda:0")
    if model is not None:
        model = model.to(dev)
    try:
        items = abx.read_items(args.item) if args.item is not None else None
        mixture = gmm.load(args.model) if args.model is not None else None
        pool = frames.pool_from_scp(args.data_format, args.feat_scp, args.len_scp, args.mvn_path, T, 1, dev)
        rows = corpus_rows(model, pool, args.on, args.batch_size)
        N, width = int(rows.shape[0]), int(rows.shape[1])
        if width > gmm.GMM_MAX_DP:
            raise ValueError("%s has %d values per frame, the mixture kernels take at most %d" % (args.on, width, gmm.GMM_MAX_DP))
        if not bool(torch.isfinite(rows).all()):
            raise ValueError("%s holds values that are not finite" % args.on)
        if mixture is None:
            mixture, hist = gmm.fit(rows, args.k, iters=args.iters, tol=args.tol, seed=args.seed, var_floor=args.var_floor,
                                    kmeans_iters=args.kmeans_iters)
        else:
            if mixture["means"].shape[1] != width:
                raise ValueError("the model is %s, but %s has %d values per frame" % (mixture["means"].shape, args.on, width))
            hist = {"mean_loglik": [], "iterations": 0, "converged": True, "starved": 0, "floored": 0}
        # through the file's own form (numpy float64), so that --model with gmm.npz repeats this run's table bit for bit
        mixture = {key: np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float64)
                   for key, v in mixture.items()}
        post, labels, _ = gmm.posteriorgram(rows, mixture, with_labels=True)
    except (ValueError, OSError, RuntimeError) as e:
        print("fit_gmm: %s" % e, file=sys.stderr)
        return 1
    if hb.lstm_sync_status() != 0:
        print("a persistent recurrence launch gave up: the results are invalid", file=sys.stderr)
        return 3
    K = int(mixture["weights"].shape[0])
    host = labels.cpu().numpy()
    ptr = pool.utt_ptr_host
    seqs = [host[int(a):int(b)] for a, b in zip(ptr[:-1], ptr[1:])]
    info = {"on": args.on, "k": K, "width": width, "frames": N, "iterations": hist["iterations"], "converged": hist["converged"],
            "mean_loglik": hist["mean_loglik"], "starved": hist["starved"], "floored": hist["floored"], "seed": int(args.seed)}
    if items is not None:
        info.update(units.bitrate(seqs, args.frame_shift))
        phones, names, overlaps = units.frame_phones(items, pool.keys, pool.lengths, args.frame_shift, args.frame_offset)
        info.update(units.unit_quality(host, phones, K, len(names)))
        info.update({"overlaps": overlaps, "phones": names})
    os.makedirs(args.out, exist_ok=True)
    gmm.save(os.path.join(args.out, "gmm.npz"), mixture)
    units.write_units(os.path.join(args.out, "units.txt"), pool.keys, seqs)
    units.write_units(os.path.join(args.out, "units_collapsed.txt"), pool.keys, [units.collapse(s) for s in seqs])
    if args.post_out is not None:
        if K > POST_MAX_SCORED:
            print("fit_gmm: the posteriorgrams have %d columns; eval_model.py's ABX and QbE take at most %d, so --baseline-feat-scp "
                  "will not score this archive under them" % (K, POST_MAX_SCORED), file=sys.stderr)
        extract_latents.write_rows(args.post_out, pool.keys, post, ptr, args.out_format, False)
    with open(os.path.join(args.out, "gmm.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps(info))
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main())
