"""probe_latents.py -- frame probes for a whole corpus: a softmax regression trained on the frame-level z1 of a trained checkpoint,
or on the input features, to predict each frame's phone or its speaker (probe.py does the work).  A good z1 gives
a high phone accuracy and a speaker accuracy near the majority baseline.

    python pytorch-scalablefhvae_amd/probe_latents.py [--checkpoint CK] --feat-scp S --len-scp S --item ITEM --out DIR
        [--data-format numpy|kaldi] [--mvn-path P] [--on z1|feats] [--target phone|speaker]
        (--holdout 0.2 [--seed 0] | --test-feat-scp S --test-len-scp S [--test-item ITEM])
        [--l2 1e-4] [--iters 200] [--gtol 1e-5] [--model FILE.npz]
        [--frame-shift 0.010] [--frame-offset 0.0] [--batch-size B] [--compute-dtype f32|bf16]

  --checkpoint CK  optional.  Without it only --on feats is allowed: the archive's rows as read (normalised by --mvn-path if given)
  --item ITEM      the alignment (abx.read_items): a frame's label is the phone, or the speaker, of the token that covers it
  --holdout H      the last ceil(H U) of RandomState(--seed).permutation(U) utterances are the test set.  With --target speaker
                   this is the only meaningful split: a test speaker has to occur in training, so a separate test corpus with
                   other speakers is refused
  --test-feat-scp  a separate test corpus (--test-item defaults to --item)
  --model FILE     score a model fitted elsewhere (probe.npz of another run) without fitting; classes and width must match
  At most 128 values per frame; a width that is no multiple of 16 is zero-padded on the device.

It writes under --out: probe.npz (weights, bias, mean, std, classes; float64), confusion.tsv (the test side, truth by rows) and
probe.json: on, target, classes, train_frames, test_frames, unlabelled, overlaps, accuracy, balanced_accuracy, majority (the test
accuracy of always answering the most frequent training class), train_accuracy, loss (nats per frame), iterations, converged, l2.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Frame probes: softmax regression on frame-level representations, on the GPU")
    p.add_argument("--checkpoint", default=None, help="optional: without it only --on feats")
    p.add_argument("--feat-scp", required=True)
    p.add_argument("--len-scp", required=True)
    p.add_argument("--item", required=True, metavar="ITEM", help="alignment with the phone and speaker of every token")
    p.add_argument("--out", required=True, help="output directory (created)")
    p.add_argument("--data-format", default="numpy", choices=["numpy", "kaldi"], help="what --feat-scp points at")
    p.add_argument("--mvn-path", default=None)
    p.add_argument("--on", default="z1", choices=["z1", "feats"], help="frame-level z1, or the normalised input features")
    p.add_argument("--target", default="phone", choices=["phone", "speaker"])
    p.add_argument("--holdout", type=float, default=None, help="share of the utterances held out as the test set (default 0.2). "
                   "With --target speaker this is the only meaningful split: every test speaker must occur in training")
    p.add_argument("--seed", type=int, default=0, help="of the --holdout permutation")
    p.add_argument("--test-feat-scp", default=None, help="a separate test corpus instead of --holdout")
    p.add_argument("--test-len-scp", default=None)
    p.add_argument("--test-item", default=None, help="default: --item")
    p.add_argument("--l2", type=float, default=1e-4)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--gtol", type=float, default=1e-5, help="stop when the gradient's infinity norm is at most this")
    p.add_argument("--model", default=None, metavar="FILE.npz", help="score this model instead of fitting one")
    p.add_argument("--frame-shift", type=float, default=0.010, help="seconds between frames")
    p.add_argument("--frame-offset", type=float, default=0.0, help="time of frame 0 in seconds")
    p.add_argument("--batch-size", type=int, default=16384, help="windows per forward")
    p.add_argument("--compute-dtype", default=None, choices=["f32", "bf16"], help="default: the checkpoint's")
    return p


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if args.checkpoint is None and args.on != "feats":
        p.error("--on %s needs --checkpoint: without --checkpoint only --on feats is possible" % args.on)
    if (args.test_feat_scp is None) != (args.test_len_scp is None):
        p.error("--test-feat-scp and --test-len-scp go together")
    if args.test_feat_scp is not None and args.holdout is not None:
        p.error("--holdout and --test-feat-scp exclude each other")
    if args.test_feat_scp is None and args.test_item is not None:
        p.error("--test-item needs --test-feat-scp")
    if args.test_feat_scp is None and args.holdout is None:
        args.holdout = 0.2
    if args.holdout is not None and not 0.0 < args.holdout < 1.0:
        p.error("--holdout %g must lie in (0, 1)" % args.holdout)
    if args.seed < 0 or args.seed >= 2 ** 32:
        p.error("--seed %d must lie in [0, 2^32)" % args.seed)
    if args.iters < 0 or args.batch_size < 1:
        p.error("--iters must not be negative and --batch-size at least 1")
    if not args.l2 >= 0 or not args.gtol >= 0:
        p.error("--l2 and --gtol must not be negative")
    if not args.frame_shift > 0:
        p.error("--frame-shift %g must be positive" % args.frame_shift)
    if args.compute_dtype is not None and args.checkpoint is None:
        p.error("--compute-dtype needs --checkpoint")
    return p, args


def write_confusion(path, names, conf):
    with open(path, "w") as f:
        f.write("truth\\predicted\t" + "\t".join(names) + "\n")
        for name, row in zip(names, conf):
            f.write(name + "\t" + "\t".join("%d" % v for v in row) + "\n")


def split_rows(rows, labels, lengths, holdout, seed):
    """(train rows, train labels, test rows, test labels) of an utterance split (probe.split_utterances), on the rows' device."""
    import torch

    import probe

    train, test = probe.split_utterances(len(lengths), holdout, seed)
    y = torch.from_numpy(labels).to(rows.device)
    a = torch.from_numpy(probe.frames_of(train, lengths)).to(rows.device)
    b = torch.from_numpy(probe.frames_of(test, lengths)).to(rows.device)
    return rows[a].contiguous(), y[a].contiguous(), rows[b].contiguous(), y[b].contiguous()


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
        print("the probe runs on a MI355X only (no CPU fallback)", file=sys.stderr)
        return 1
    import abx
    import frames
    import hip_binding as hb
    import probe
    from fit_gmm import corpus_rows

    dev = torch.device("cuda:0")
    if model is not None:
        model = model.to(dev)
    try:
        items = abx.read_items(args.item)
        fitted = probe.load(args.model) if args.model is not None else None
        pool = frames.pool_from_scp(args.data_format, args.feat_scp, args.len_scp, args.mvn_path, T, 1, dev)
        rows = corpus_rows(model, pool, args.on, args.batch_size)
        if int(rows.shape[1]) > probe.PROBE_MAX_W:
            raise ValueError("%s has %d values per frame, the probe kernels take at most %d" % (args.on, rows.shape[1], probe.PROBE_MAX_W))
        labels, names, overlaps = probe.frame_labels(items, pool.keys, pool.lengths, args.target, args.frame_shift, args.frame_offset)
        if args.test_feat_scp is None:
            train_x, train_y, test_x, test_y = split_rows(rows, labels, pool.lengths, args.holdout, args.seed)
        else:
            test_items = abx.read_items(args.test_item) if args.test_item is not None else items
            tpool = frames.pool_from_scp(args.data_format, args.test_feat_scp, args.test_len_scp, args.mvn_path, T, 1, dev)
            test_x = corpus_rows(model, tpool, args.on, args.batch_size)
            tl, tnames, tover = probe.frame_labels(test_items, tpool.keys, tpool.lengths, args.target, args.frame_shift, args.frame_offset)
            overlaps += tover
            new = [n for n in tnames if n not in names]
            if new and args.target == "speaker":
                raise ValueError("test speaker %s never occurs in training: a speaker probe needs the same speakers on both sides "
                                 "(use --holdout)" % new[0])
            names = names + new  # (a phone the training side lacks keeps weights 0)
            remap = np.array([names.index(n) for n in tnames] + [-1], dtype=np.int32)
            train_x, train_y = rows, torch.from_numpy(labels).to(dev)
            test_y = torch.from_numpy(remap[tl]).to(dev)
        if not names:
            raise ValueError("no frame of --feat-scp lies under a token of %s" % args.item)
        if args.target == "speaker" and args.test_feat_scp is None:
            seen = set(train_y[train_y >= 0].unique().tolist())
            lost = [names[c] for c in test_y[test_y >= 0].unique().tolist() if c not in seen]
            if lost:
                raise ValueError("test speaker %s never occurs in training under --holdout %g --seed %d" % (lost[0], args.holdout, args.seed))
        fitted, report, conf = probe.run(train_x, train_y, test_x, test_y, names, args.l2, args.iters, args.gtol, fitted)
    except (ValueError, OSError, RuntimeError) as e:
        print("probe_latents: %s" % e, file=sys.stderr)
        return 1
    if hb.lstm_sync_status() != 0:
        print("a persistent recurrence launch gave up: the results are invalid", file=sys.stderr)
        return 3
    unlabelled = int((train_y < 0).sum()) + int((test_y < 0).sum())
    info = {"on": args.on, "target": args.target}
    info.update(report)
    info.update({"unlabelled": unlabelled, "overlaps": int(overlaps)})
    order = ("on", "target", "classes", "train_frames", "test_frames", "unlabelled", "overlaps", "accuracy", "balanced_accuracy", "majority",
             "train_accuracy", "loss", "iterations", "converged", "l2")
    info = {k: info[k] for k in order}
    os.makedirs(args.out, exist_ok=True)
    probe.save(os.path.join(args.out, "probe.npz"), fitted)
    write_confusion(os.path.join(args.out, "confusion.tsv"), names, conf)
    with open(os.path.join(args.out, "probe.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps(info))
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main())
