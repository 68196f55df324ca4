"""discover_units.py -- discrete acoustic units for a whole corpus: a k-means codebook on the frame-level z1 of a trained
checkpoint (or on the input features, the baseline), one unit per frame (units.py does the work; DESIGN.md, "Units").

    python pytorch-scalablefhvae_amd/discover_units.py --checkpoint CK --feat-scp S --len-scp S [--data-format numpy|kaldi]
        [--mvn-path P] --out DIR (--k K | --codebook FILE.npy) [--on z1|feats] [--iters 100] [--tol 1e-4] [--n-init 1] [--seed 0]
        [--batch-size B] [--compute-dtype f32|bf16] [--item FILE [--frame-shift 0.010] [--frame-offset 0.0]]
        [--segment [--dur-penalty LAMBDA] [--max-seg-frames L] [--boundary-tol 0.020]]

  --k K            fit K centroids on this corpus (units.fit: Lloyd's algorithm from K rows drawn with --seed)
  --codebook FILE  apply a (K, width) table fitted elsewhere (units_centroids.npy of another run); the width must match
  --on z1          frames.encode_frames at shift 1: row f is frame f.  --on feats: the normalised input; a width that is no
                   multiple of 16 is zero-padded on the device, one above 128 is an error
  --item FILE      a phone alignment (abx.read_items): cluster purity, phone purity and PNMI of the units against it
  --segment        also cut every utterance into segments of at most --max-seg-frames frames, one unit each, that minimise the
                   quantisation error plus --dur-penalty per segment (segment.py)

It writes under --out: units_centroids.npy (K, width), units_counts.npy (K,), units.txt and units_collapsed.txt (one line
`key u0 u1 ...` per utterance in --feat-scp order; collapsed: runs of equal units merged) and units.json: on, k, frames,
iterations, converged, inertia, reseeded, seed, bitrate, bitrate_collapsed and, with --item, cluster_purity, phone_purity, pnmi,
labelled_frames, overlaps and phones.  With --segment also segments.item (one item per segment, #phone `u<k>`), segments.txt
(`key u0 u1 ...`, one unit per segment) and in units.json "segments": dur_penalty, max_seg_frames, segments, mean_frames, cost,
bitrate_segments and, with --item, precision, recall, f, os, r_value of the boundaries (within --boundary-tol seconds), their
counts, and cluster_purity, phone_purity, pnmi of the segments' units per frame.  Without --segment nothing changes.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Discrete acoustic units: k-means on frame-level latents, on the GPU")
    p.add_argument("--checkpoint", required=True)
    p.add_argument("--feat-scp", required=True)
    p.add_argument("--len-scp", required=True)
    p.add_argument("--data-format", default="numpy", choices=["numpy", "kaldi"], help="what --feat-scp points at")
    p.add_argument("--mvn-path", default=None)
    p.add_argument("--out", required=True, help="output directory (created)")
    how = p.add_mutually_exclusive_group(required=True)
    how.add_argument("--k", type=int, default=None, help="fit this many centroids on the corpus")
    how.add_argument("--codebook", default=None, metavar="FILE.npy", help="apply this (K, width) table instead of fitting one")
    p.add_argument("--on", default="z1", choices=["z1", "feats"], help="frame-level z1, or the normalised input features")
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--tol", type=float, default=1e-4, help="stop when the inertia falls by less than this share")
    p.add_argument("--n-init", type=int, default=1, help="restarts (seeds --seed, --seed + 1, ...); the lowest inertia wins")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--batch-size", type=int, default=16384, help="windows per forward")
    p.add_argument("--compute-dtype", default=None, choices=["f32", "bf16"], help="default: the checkpoint's")
    p.add_argument("--item", default=None, metavar="FILE", help="phone alignment to score the units against")
    p.add_argument("--frame-shift", type=float, default=0.010, help="seconds between frames")
    p.add_argument("--frame-offset", type=float, default=0.0, help="time of frame 0 in seconds")
    p.add_argument("--segment", action="store_true", help="also segment every utterance over the codebook (segment.py)")
    p.add_argument("--dur-penalty", type=float, default=1.0, metavar="LAMBDA", help="--segment: the penalty per segment")
    p.add_argument("--max-seg-frames", type=int, default=32, metavar="L", help="--segment: frames per segment, at most (1 .. 64)")
    p.add_argument("--boundary-tol", type=float, default=0.020, help="--segment with --item: seconds within which a boundary is hit")
    return p


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if args.k is not None and args.k < 1:
        p.error("--k %d must be at least 1" % args.k)
    if args.iters < 1 or args.n_init < 1 or args.batch_size < 1:
        p.error("--iters, --n-init and --batch-size must be at least 1")
    if args.seed < 0 or args.seed + args.n_init > 2 ** 32:
        p.error("--seed %d (+ --n-init) must lie in [0, 2^32)" % args.seed)
    if not args.frame_shift > 0:
        p.error("--frame-shift %g must be positive" % args.frame_shift)
    if not args.dur_penalty >= 0 or not 1 <= args.max_seg_frames <= 64 or not args.boundary_tol >= 0:
        p.error("--dur-penalty and --boundary-tol must be at least 0 and --max-seg-frames lie in [1, 64]")
    return p, args


def main(argv=None) -> int:
    parser, args = parse_args(argv)
    import torch

    import utils

    model = utils.load_checkpoint_file(args.checkpoint, finetune=True)[0].eval()
    T = int(getattr(model, "seg_len", 20))
    if args.compute_dtype is not None:
        if not hasattr(model, "compute_dtype"):
            parser.error("--compute-dtype: a %s checkpoint computes in f32 only" % model.model)
        model.compute_dtype = args.compute_dtype
    if not torch.cuda.is_available():
        print("unit discovery runs on a MI355X only (no CPU fallback)", file=sys.stderr)
        return 1
    import abx
    import frames
    import hip_binding as hb
    import units

    dev = torch.device("cuda:0")
    model = model.to(dev)
    try:
        items = abx.read_items(args.item) if args.item is not None else None
        codebook = np.load(args.codebook) if args.codebook is not None else None
        pool = frames.pool_from_scp(args.data_format, args.feat_scp, args.len_scp, args.mvn_path, T, 1, dev)
        rows, width = units.corpus_rows(model, pool, args.on, args.batch_size)
        info, cent, counts, seqs = units.discover(rows, width, pool.keys, pool.lengths, args.on, k=args.k, codebook=codebook,
                                                  iters=args.iters, tol=args.tol, n_init=args.n_init, seed=args.seed, items=items,
                                                  frame_shift=args.frame_shift, frame_offset=args.frame_offset)
        if args.segment:
            import segment

            info["segments"], segs, seg_items = segment.discover(rows, cent, pool.keys, pool.lengths, args.dur_penalty, args.max_seg_frames,
                                                                 info["k"], items=items, frame_shift=args.frame_shift,
                                                                 frame_offset=args.frame_offset, tol=args.boundary_tol)
    except (ValueError, OSError) as e:
        print("discover_units: %s" % e, file=sys.stderr)
        return 1
    if hb.lstm_sync_status() != 0:
        print("a persistent recurrence launch gave up: the results are invalid", file=sys.stderr)
        return 3
    os.makedirs(args.out, exist_ok=True)
    np.save(os.path.join(args.out, "units_centroids.npy"), cent)
    np.save(os.path.join(args.out, "units_counts.npy"), counts)
    units.write_units(os.path.join(args.out, "units.txt"), pool.keys, seqs)
    units.write_units(os.path.join(args.out, "units_collapsed.txt"), pool.keys, [units.collapse(s) for s in seqs])
    if args.segment:
        abx.write_items(os.path.join(args.out, "segments.item"), seg_items)
        units.write_units(os.path.join(args.out, "segments.txt"), pool.keys, [un for _, un in segs])
    with open(os.path.join(args.out, "units.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps(info))
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main())
