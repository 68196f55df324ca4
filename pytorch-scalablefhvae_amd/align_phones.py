"""align_phones.py -- forced alignment for a whole corpus: a transcription per utterance (the token order, no times) and per-frame
scores of a linear model on the frame-level z1 of a trained checkpoint, or on the input features, give back the first and last
frame of every token, written as an item file that eval_model.py --abx-item / --probe-item / --per-item / --units-item,
probe_latents.py and recognise_phones.py read (falign.py does the work).

    python pytorch-scalablefhvae_amd/align_phones.py [--checkpoint CK] --feat-scp S --len-scp S (--text FILE | --item ITEM) --out DIR
        [--data-format numpy|kaldi] [--mvn-path P] [--on z1|feats] [--topology ctc|hmm] [--model FILE.npz --phones FILE]
        [--ctc-context K] [--l2 1e-4] [--iters 200] [--gtol 1e-5] [--blank-rule follow|own]
        [--utt2spk FILE | --spk-key-sep SEP] [--ref-item ITEM] [--frame-shift 0.010] [--frame-offset 0.0]
        [--batch-size B] [--compute-dtype f32|bf16]

  --checkpoint CK  optional.  Without it only --on feats is allowed: the archive's rows as read
  --text FILE      Kaldi's `text`: `key tok tok ...`; a line with a key only is an empty transcription
  --item ITEM      an item file read for its token order only (phonerec.references); its times play no part
  --topology ctc   (default) blank between the tokens.  Without --model a linear CTC model is fitted on the transcriptions given
                   (ctc.fit, --ctc-context frames spliced per side) and written as ctc.npz with phones.txt, the class names in
                   order; with --model FILE.npz (ctc.npz of another run) and --phones FILE that model is taken
  --topology hmm   one state per token, no blank: needs --model (a probe.npz of probe_latents.py / recognise_phones.py) and --phones
  --blank-rule     follow (default): a token runs to the frame before the next token's first, the last one to the end; own: the
                   frames of the token's own state only.  The HMM topology has no blank and both give the same
  --ref-item ITEM  a time-aligned reference: align.json gets falign.boundary_report against it
  An utterance of --feat-scp without a transcription, or with a token the model does not know, is `unknown`; one whose
  transcription has no path (too few frames, more than 256 tokens) is `infeasible`.  Both are counted, named on stderr and listed
  in align.json; neither is dropped silently.  The speaker column is `-` without --utt2spk / --spk-key-sep.

It writes under --out: aligned.item and align.json: topology, blank_rule, on, utterances, aligned, tokens, infeasible and unknown
(the keys), mean_path_logprob_per_frame (the best paths' log-probability under the row-wise softmax, per aligned frame), the
settings, with a fitted model objective / iterations / converged / context, and with --ref-item "boundaries".
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Forced alignment of transcriptions to frame-level representations on the GPU")
    p.add_argument("--checkpoint", default=None, help="optional: without it only --on feats")
    p.add_argument("--feat-scp", required=True)
    p.add_argument("--len-scp", required=True)
    p.add_argument("--data-format", default="numpy", choices=["numpy", "kaldi"], help="what --feat-scp points at")
    p.add_argument("--mvn-path", default=None)
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--text", default=None, metavar="FILE", help="Kaldi text: `key tok tok ...`")
    src.add_argument("--item", default=None, metavar="ITEM", help="an item file, read for its token order only")
    p.add_argument("--out", required=True, help="output directory (created)")
    p.add_argument("--on", default="z1", choices=["z1", "feats"], help="frame-level z1, or the normalised input features")
    p.add_argument("--topology", default="ctc", choices=["ctc", "hmm"])
    p.add_argument("--model", default=None, metavar="FILE.npz", help="ctc.npz (topology ctc) or probe.npz (topology hmm)")
    p.add_argument("--phones", default=None, metavar="FILE", help="the model's class names, one per line, in order")
    p.add_argument("--ctc-context", type=int, default=0, metavar="K", help="frames spliced per side when a CTC model is fitted")
    p.add_argument("--l2", type=float, default=1e-4)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--gtol", type=float, default=1e-5, help="stop when the gradient's infinity norm is at most this")
    p.add_argument("--blank-rule", default="follow", choices=["follow", "own"])
    spk = p.add_mutually_exclusive_group()
    spk.add_argument("--utt2spk", default=None, help="Kaldi utt2spk file naming each utterance's speaker")
    spk.add_argument("--spk-key-sep", default=None, help="the speaker is the key up to the first SEP")
    p.add_argument("--ref-item", default=None, metavar="ITEM", help="a time-aligned reference for the boundary report")
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
    if (args.model is None) != (args.phones is None):
        p.error("--model and --phones go together")
    if args.topology == "hmm" and args.model is None:
        p.error("--topology hmm needs --model (a probe .npz) and --phones")
    if args.ctc_context < 0 or (args.ctc_context != 0 and (args.model is not None or args.topology != "ctc")):
        p.error("--ctc-context must not be negative and applies only where a CTC model is fitted")
    if args.iters < 0 or args.batch_size < 1:
        p.error("--iters must not be negative and --batch-size at least 1")
    if not args.l2 >= 0 or not args.gtol >= 0:
        p.error("--l2 and --gtol must not be negative")
    if not args.frame_shift > 0:
        p.error("--frame-shift %g must be positive" % args.frame_shift)
    if args.compute_dtype is not None and args.checkpoint is None:
        p.error("--compute-dtype needs --checkpoint")
    return p, args


def read_phones(path):
    with open(path) as fh:
        names = [line.split()[0] for line in fh if line.split()]
    if not names or len(set(names)) != len(names):
        raise ValueError("%s: the class names must be at least one and differ" % path)
    return names


def transcriptions(args, keys):
    """-> for every key of the corpus its list of token names, or None where the source holds no transcription of it."""
    import abx
    import falign
    import phonerec

    if args.text is not None:
        table = dict(zip(*falign.read_text(args.text)))
        return [table.get(k) for k in keys]
    refs = phonerec.references(abx.read_items(args.item), keys)
    return [r if r else None for r in refs]  # (an item file cannot say "this utterance is empty")


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
        print("forced alignment runs on a MI355X only (no CPU fallback)", file=sys.stderr)
        return 1
    import abx
    import ctc
    import falign
    import frames
    import hip_binding as hb
    import phonerec
    import probe
    import verification
    from fit_gmm import corpus_rows

    dev = torch.device("cuda:0")
    if model is not None:
        model = model.to(dev)
    fit_info = {}
    try:
        pool = frames.pool_from_scp(args.data_format, args.feat_scp, args.len_scp, args.mvn_path, T, 1, dev)
        keys, lengths = list(pool.keys), np.asarray(pool.lengths, dtype=np.int64)
        rows = corpus_rows(model, pool, args.on, args.batch_size)
        if int(rows.shape[1]) > probe.PROBE_MAX_W:
            raise ValueError("%s has %d values per frame, the kernels take at most %d" % (args.on, rows.shape[1], probe.PROBE_MAX_W))
        toks = transcriptions(args, keys)
        if args.utt2spk is not None:
            table = verification.read_utt2spk(args.utt2spk)
            speakers = [table.get(k, "-") for k in keys]
        elif args.spk_key_sep is not None:
            speakers = verification.speakers_from_keys(keys, args.spk_key_sep)
        else:
            speakers = ["-"] * len(keys)
        fitted = None
        if args.model is not None:
            names = read_phones(args.phones)
            fitted = ctc.load(args.model) if args.topology == "ctc" else probe.load(args.model)
            n_rows = int(fitted["weights"].shape[0])
            if n_rows != len(names) + (args.topology == "ctc"):
                raise ValueError("%s has %d classes, %s names %d%s" % (args.model, n_rows, args.phones, len(names),
                                                                       " (and the blank)" if args.topology == "ctc" else ""))
            if args.topology == "ctc" and int(fitted["blank"]) != len(names):
                raise ValueError("%s: the blank is class %d, not the last" % (args.model, int(fitted["blank"])))
        else:
            names = sorted({t for ref in toks if ref is not None for t in ref})
            if not names:
                raise ValueError("no utterance of --feat-scp has a transcription with a token")
        index = {n: i for i, n in enumerate(names)}
        used = [u for u, ref in enumerate(toks) if ref is not None and all(t in index for t in ref)]
        known = set(used)
        unknown = [keys[u] for u in range(len(keys)) if u not in known]
        if not used:
            raise ValueError("no utterance of --feat-scp has a transcription")
        refs = [[index[t] for t in toks[u]] for u in used]
        x = rows if len(used) == len(keys) else rows[torch.from_numpy(probe.frames_of(used, lengths)).to(dev)].contiguous()
        ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths[used])]).astype(np.int64)).to(dev)
        if fitted is None:
            fitted, hist = ctc.fit(x, ptr, refs, len(names), l2=args.l2, iters=args.iters, gtol=args.gtol, context=args.ctc_context)
            fit_info = {"objective": float(hist["objective"][-1]), "iterations": int(hist["iterations"]), "converged": bool(hist["converged"]),
                        "context": int(args.ctc_context), "dropped_infeasible": int(hist["dropped_infeasible"]), "l2": float(args.l2)}
        blank = int(fitted["blank"]) if args.topology == "ctc" else -1
        scores = falign.scores_of(x, ptr, fitted)
        labels, lab_ptr = phonerec.csr(refs, dev)
        state, seg, score, bits = falign.align(scores, ptr, labels, lab_ptr, blank)
        sp = falign.spans(seg, lab_ptr, lengths[used], args.blank_rule if args.topology == "ctc" else "own")
        logp = falign.path_logprob(scores, ptr, score).cpu().numpy()
        out_items = falign.items([keys[u] for u in used], [speakers[u] for u in used], sp, refs, names, args.frame_shift, args.frame_offset)
        report = None
        if args.ref_item is not None:
            report = falign.boundary_report(out_items, abx.read_items(args.ref_item), args.frame_shift)
    except (ValueError, OSError, RuntimeError) as e:
        print("align_phones: %s" % e, file=sys.stderr)
        return 1
    if hb.lstm_sync_status() != 0:
        print("a persistent recurrence launch gave up: the results are invalid", file=sys.stderr)
        return 3
    done = np.isfinite(logp)
    infeasible = [keys[u] for u, ok in zip(used, done) if not ok]
    for what, bad in (("infeasible", infeasible), ("unknown", unknown)):
        if bad:
            print("align_phones: %d %s utterance(s): %s" % (len(bad), what, " ".join(bad)), file=sys.stderr)
    n_frames = int(lengths[used][done].sum())
    info = {"topology": args.topology, "blank_rule": args.blank_rule if args.topology == "ctc" else "own", "on": args.on,
            "utterances": len(keys), "aligned": int(done.sum()), "tokens": len(out_items), "infeasible": infeasible, "unknown": unknown,
            "mean_path_logprob_per_frame": float(logp[done].sum()) / n_frames if n_frames else None, "classes": names,
            "frame_shift": args.frame_shift, "frame_offset": args.frame_offset, "model": args.model}
    info.update(fit_info)
    if report is not None:
        info["boundaries"] = report
    os.makedirs(args.out, exist_ok=True)
    abx.write_items(os.path.join(args.out, "aligned.item"), out_items)
    if args.model is None:
        ctc.save(os.path.join(args.out, "ctc.npz"), fitted)
        with open(os.path.join(args.out, "phones.txt"), "w") as f:
            f.write("".join(n + "\n" for n in names))
    with open(os.path.join(args.out, "align.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps(info))
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main())
