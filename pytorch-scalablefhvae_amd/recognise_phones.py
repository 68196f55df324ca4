"""recognise_phones.py -- phone recognition for a whole corpus: a frame probe on the frame-level z1 of a trained checkpoint, or on
the input features, gives per-frame phone scores; a Viterbi pass under a frame-level phone bigram turns them into a phone
sequence, which is scored against the transcription by the phone error rate (phonerec.py does the work).

    python pytorch-scalablefhvae_amd/recognise_phones.py [--checkpoint CK] --feat-scp S --len-scp S --item ITEM --out DIR
        (--holdout 0.2 [--seed 0] | --test-feat-scp S --test-len-scp S [--test-item ITEM])
        [--data-format numpy|kaldi] [--mvn-path P] [--on z1|feats] [--probe FILE.npz] [--phone-map FILE]
        [--acoustic-scale 1] [--prior-scale 1] [--phone-penalty 0] [--smooth 1]
        [--l2 1e-4] [--iters 200] [--gtol 1e-5] [--frame-shift 0.010] [--frame-offset 0.0] [--batch-size B]
        [--compute-dtype f32|bf16] [--ctc [--ctc-context K] [--ctc-init zero|probe]
        [--ctc-beam W [--ctc-lm-scale S --ctc-bonus B | --ctc-lm-tune] [--ctc-class-beam G] [--ctc-lm-smooth A]]]

  --checkpoint CK  optional.  Without it only --on feats is allowed: the archive's rows as read (the MFCC baseline)
  --item ITEM      the alignment (abx.read_items): it labels the training frames and, in onset order, is the transcription.  An
                   alignment that leaves out tokens (a silence, the first and last phone of a file) makes every hypothesis phone
                   over them an insertion: tools/timit_items.py --tier phn-all writes every phone
  --probe FILE     take this model (probe.npz of another run) instead of fitting one; classes and width must match
  --phone-map FILE lines `phone target`, a target `-` deletes: both the reference and the hypothesis are mapped after decoding
                   (TIMIT: the 61 -> 39 fold with q deleted); two neighbours that fold together stay two tokens
  --phone-penalty P  subtracted from every transition between two different phones (the insertion penalty)
  --ctc            beside everything above, train the same linear model by CTC (ctc.py) on the transcriptions of
                   the training utterances alone (phonerec.references: the token order; the item's times play no part) and decode
                   the test utterances greedily.  --ctc-context K splices K frames per side; --ctc-init probe starts from the
                   frame probe's rows (context 0 only).  At most 127 phones; an utterance without an alignment is dropped
  At most 128 phones and 128 values per frame; a reference of at most 256 tokens.

It writes under --out: probe.npz, hyp.txt and ref.txt (`key p1 p2 ...`, folded) and phonerec.json: on, per, sub, del, ins, cor,
ref_tokens, utterances, per_argmax (the collapsed per-frame arg-max instead of the Viterbi path), frame_accuracy,
frame_accuracy_argmax, classes, folded_classes, train_frames, test_frames, iterations, converged and the settings.
With --ctc --ctc-beam W also hyp_ctc_beam.txt, ctc_lm.npy (the bigram of the training transcriptions, ctcbeam.bigram) and a
"ctc_beam" block: the error rate's keys, beam, lm_scale, bonus, class_beam, smooth and the tuning grid (null unless --ctc-lm-tune).
With --ctc also ctc.npz and hyp_ctc.txt, and a "ctc" block in phonerec.json: per, sub, del, ins, cor, objective, iterations,
converged, context, dropped_infeasible (and ref_tokens, utterances, l2, init).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Phone recognition on frame-level representations: Viterbi decoding and PER on the GPU")
    p.add_argument("--checkpoint", default=None, help="optional: without it only --on feats")
    p.add_argument("--feat-scp", required=True)
    p.add_argument("--len-scp", required=True)
    p.add_argument("--item", required=True, metavar="ITEM", help="alignment: the training labels and the transcription")
    p.add_argument("--out", required=True, help="output directory (created)")
    p.add_argument("--data-format", default="numpy", choices=["numpy", "kaldi"], help="what --feat-scp points at")
    p.add_argument("--mvn-path", default=None)
    p.add_argument("--on", default="z1", choices=["z1", "feats"], help="frame-level z1, or the normalised input features")
    p.add_argument("--holdout", type=float, default=None, help="share of the utterances held out as the test set (default 0.2)")
    p.add_argument("--seed", type=int, default=0, help="of the --holdout permutation")
    p.add_argument("--test-feat-scp", default=None, help="a separate test corpus instead of --holdout")
    p.add_argument("--test-len-scp", default=None)
    p.add_argument("--test-item", default=None, help="default: --item")
    p.add_argument("--probe", default=None, metavar="FILE.npz", help="take this probe model instead of fitting one")
    p.add_argument("--phone-map", default=None, metavar="FILE", help="lines `phone target`; a target `-` deletes the phone")
    p.add_argument("--acoustic-scale", type=float, default=1.0)
    p.add_argument("--prior-scale", type=float, default=1.0)
    p.add_argument("--phone-penalty", type=float, default=0.0, help="subtracted from every transition between different phones")
    p.add_argument("--smooth", type=float, default=1.0, help="added to every bigram count")
    p.add_argument("--l2", type=float, default=1e-4)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--gtol", type=float, default=1e-5, help="stop when the gradient's infinity norm is at most this")
    p.add_argument("--frame-shift", type=float, default=0.010, help="seconds between frames")
    p.add_argument("--frame-offset", type=float, default=0.0, help="time of frame 0 in seconds")
    p.add_argument("--batch-size", type=int, default=16384, help="windows per forward")
    p.add_argument("--compute-dtype", default=None, choices=["f32", "bf16"], help="default: the checkpoint's")
    p.add_argument("--ctc", action="store_true", help="also train by CTC on the transcriptions alone and decode greedily")
    p.add_argument("--ctc-context", type=int, default=0, metavar="K", help="frames spliced per side")
    p.add_argument("--ctc-init", default="zero", choices=["zero", "probe"], help="start from zero or from the frame probe's rows")
    p.add_argument("--ctc-beam", type=int, default=None, metavar="W", help="with --ctc: also decode by prefix beam search of this width with a phone bigram (ctcbeam.py)")
    p.add_argument("--ctc-lm-scale", type=float, default=None, metavar="S", help="the bigram's weight (default 1)")
    p.add_argument("--ctc-bonus", type=float, default=None, metavar="B", help="added per phone put out (default 0)")
    p.add_argument("--ctc-lm-tune", action="store_true", help="choose the weight and the bonus on the training utterances instead")
    p.add_argument("--ctc-class-beam", type=float, default=float("inf"), metavar="G", help="classes further than this below the frame's best are not extended into")
    p.add_argument("--ctc-lm-smooth", type=float, default=1.0, metavar="A", help="added to every bigram count")
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
    if not args.l2 >= 0 or not args.gtol >= 0 or not args.smooth >= 0:
        p.error("--l2, --gtol and --smooth must not be negative")
    if not args.acoustic_scale > 0 or not args.prior_scale >= 0 or not np.isfinite(args.phone_penalty):
        p.error("--acoustic-scale must be positive, --prior-scale not negative and --phone-penalty finite")
    if not args.frame_shift > 0:
        p.error("--frame-shift %g must be positive" % args.frame_shift)
    if args.compute_dtype is not None and args.checkpoint is None:
        p.error("--compute-dtype needs --checkpoint")
    if not args.ctc and (args.ctc_context != 0 or args.ctc_init != "zero"):
        p.error("--ctc-context and --ctc-init need --ctc")
    if args.ctc_context < 0 or (args.ctc_init == "probe" and args.ctc_context != 0):
        p.error("--ctc-context must not be negative, and --ctc-init probe needs --ctc-context 0")
    beam_flags = args.ctc_lm_scale is not None or args.ctc_bonus is not None or args.ctc_lm_tune or args.ctc_class_beam != float("inf") or args.ctc_lm_smooth != 1.0
    if args.ctc_beam is None and beam_flags:
        p.error("--ctc-lm-scale, --ctc-bonus, --ctc-lm-tune, --ctc-class-beam and --ctc-lm-smooth need --ctc-beam")
    if args.ctc_beam is not None and (not args.ctc or not 1 <= args.ctc_beam <= 64):
        p.error("--ctc-beam needs --ctc and a width from 1 to 64")
    if args.ctc_lm_tune and (args.ctc_lm_scale is not None or args.ctc_bonus is not None):
        p.error("--ctc-lm-tune excludes --ctc-lm-scale and --ctc-bonus")
    if (args.ctc_lm_scale is not None and not 0 <= args.ctc_lm_scale < float("inf")) or (args.ctc_bonus is not None and not np.isfinite(args.ctc_bonus)):
        p.error("--ctc-lm-scale must be finite and not negative, --ctc-bonus finite")
    if not args.ctc_class_beam >= 0 or not args.ctc_lm_smooth >= 0:
        p.error("--ctc-class-beam and --ctc-lm-smooth must not be negative")
    return p, args


def reference_ids(refs, names):
    """Lists of phone names -> lists of ids into `names`; a phone that labels no frame is appended to `names`."""
    index = {n: i for i, n in enumerate(names)}
    out = []
    for ref in refs:
        for ph in ref:
            if ph not in index:
                index[ph] = len(names)
                names.append(ph)
        out.append([index[ph] for ph in ref])
    return out


def split_corpus(rows, labels, lengths, refs, keys, holdout, seed):
    """The utterance split of probe.split_utterances -> (train rows, labels, lengths), (test rows, labels, lengths, refs, keys)."""
    import torch

    import probe

    train, test = probe.split_utterances(len(lengths), holdout, seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    y = torch.from_numpy(labels).to(rows.device)
    a = torch.from_numpy(probe.frames_of(train, lengths)).to(rows.device)
    b = torch.from_numpy(probe.frames_of(test, lengths)).to(rows.device)
    return ((rows[a].contiguous(), y[a].contiguous(), lengths[train]),
            (rows[b].contiguous(), y[b].contiguous(), lengths[test], [refs[u] for u in test], [keys[u] for u in test]))


def write_tokens(path, keys, seqs, names):
    with open(path, "w") as f:
        for key, seq in zip(keys, seqs):
            f.write(" ".join([key] + [names[t] for t in seq]) + "\n")


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
        print("phone recognition runs on a MI355X only (no CPU fallback)", file=sys.stderr)
        return 1
    import abx
    import frames
    import hip_binding as hb
    import phonerec
    import probe
    from fit_gmm import corpus_rows

    dev = torch.device("cuda:0")
    if model is not None:
        model = model.to(dev)
    try:
        items = abx.read_items(args.item)
        fitted = probe.load(args.probe) if args.probe is not None else None
        pool = frames.pool_from_scp(args.data_format, args.feat_scp, args.len_scp, args.mvn_path, T, 1, dev)
        rows = corpus_rows(model, pool, args.on, args.batch_size)
        if int(rows.shape[1]) > probe.PROBE_MAX_W:
            raise ValueError("%s has %d values per frame, the probe kernels take at most %d" % (args.on, rows.shape[1], probe.PROBE_MAX_W))
        labels, names, _ = probe.frame_labels(items, pool.keys, pool.lengths, "phone", args.frame_shift, args.frame_offset)
        if not names:
            raise ValueError("no frame of --feat-scp lies under a token of %s" % args.item)
        refs = reference_ids(phonerec.references(items, pool.keys), names)
        train_refs = refs
        if args.test_feat_scp is None:
            train, test = split_corpus(rows, labels, pool.lengths, refs, pool.keys, args.holdout, args.seed)
            train_refs = [refs[u] for u in probe.split_utterances(len(pool.lengths), args.holdout, args.seed)[0]]
        else:
            test_items = abx.read_items(args.test_item) if args.test_item is not None else items
            tpool = frames.pool_from_scp(args.data_format, args.test_feat_scp, args.test_len_scp, args.mvn_path, T, 1, dev)
            test_x = corpus_rows(model, tpool, args.on, args.batch_size)
            tl, tnames, _ = probe.frame_labels(test_items, tpool.keys, tpool.lengths, "phone", args.frame_shift, args.frame_offset)
            names = names + [n for n in tnames if n not in names]  # (a phone the training side lacks keeps weights 0)
            remap = np.array([names.index(n) for n in tnames] + [-1], dtype=np.int32)
            test_refs = reference_ids(phonerec.references(test_items, tpool.keys), names)
            train = (rows, torch.from_numpy(labels).to(dev), np.asarray(pool.lengths, dtype=np.int64))
            test = (test_x, torch.from_numpy(remap[tl]).to(dev), np.asarray(tpool.lengths, dtype=np.int64), test_refs, list(tpool.keys))
        table, folded = np.arange(len(names), dtype=np.int32), list(names)
        if args.phone_map is not None:
            table, folded = phonerec.read_phone_map(args.phone_map, names)
        fitted, report, hyp, ref = phonerec.recognise(train[0], train[1], train[2], test[0], test[2], test[3], names, l2=args.l2,
                                                      iters=args.iters, gtol=args.gtol, model=fitted, smooth=args.smooth,
                                                      penalty=args.phone_penalty, acoustic_scale=args.acoustic_scale,
                                                      prior_scale=args.prior_scale, phone_table=table, test_y=test[1])
        ctc_out = None
        if args.ctc:
            import ctc

            ctc_out = ctc.recognise(train[0], train[2], train_refs, test[0], test[2], test[3], names, l2=args.l2, iters=args.iters,
                                    gtol=args.gtol, context=args.ctc_context, init=fitted if args.ctc_init == "probe" else None,
                                    phone_table=table)
            beam_out = None
            if args.ctc and args.ctc_beam is not None:
                import ctcbeam

                tuned = args.ctc_lm_tune
                beam_out = ctcbeam.recognise(train[0], train[2], train_refs, test[0], test[2], test[3], names, beam=args.ctc_beam,
                                             scale=None if tuned else (1.0 if args.ctc_lm_scale is None else args.ctc_lm_scale),
                                             bonus=None if tuned else (0.0 if args.ctc_bonus is None else args.ctc_bonus),
                                             class_beam=args.ctc_class_beam, smooth=args.ctc_lm_smooth, phone_table=table, model=ctc_out[0])
    except (ValueError, OSError, RuntimeError) as e:
        print("recognise_phones: %s" % e, file=sys.stderr)
        return 1
    if hb.lstm_sync_status() != 0:
        print("a persistent recurrence launch gave up: the results are invalid", file=sys.stderr)
        return 3
    info = {"on": args.on}
    info.update(report)
    info.update({"folded_classes": folded, "train_frames": int((train[1] >= 0).sum()), "holdout": args.holdout, "seed": args.seed,
                 "frame_shift": args.frame_shift, "frame_offset": args.frame_offset, "phone_map": args.phone_map})
    os.makedirs(args.out, exist_ok=True)
    probe.save(os.path.join(args.out, "probe.npz"), fitted)
    write_tokens(os.path.join(args.out, "hyp.txt"), test[4], hyp, folded)
    write_tokens(os.path.join(args.out, "ref.txt"), test[4], ref, folded)
    if ctc_out is not None:
        info["ctc"] = dict(ctc_out[1], init=args.ctc_init)
        ctc.save(os.path.join(args.out, "ctc.npz"), ctc_out[0])
        write_tokens(os.path.join(args.out, "hyp_ctc.txt"), test[4], ctc_out[2], folded)
        if beam_out is not None:
            info["ctc_beam"] = beam_out[1]
            write_tokens(os.path.join(args.out, "hyp_ctc_beam.txt"), test[4], beam_out[2], folded)
            np.save(os.path.join(args.out, "ctc_lm.npy"), beam_out[4])
    with open(os.path.join(args.out, "phonerec.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps(info))
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main())
