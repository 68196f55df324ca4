"""extract_latents.py -- apply a trained checkpoint to a whole corpus and write the results as archives the project's own
datasets read back (frames.py does the work; DESIGN.md, "Frame-level latents").

    python pytorch-scalablefhvae_amd/extract_latents.py --checkpoint CK --feat-scp S --len-scp S [--data-format numpy|kaldi]
        [--mvn-path P] --out DIR --what z1 mu2 recon convert [--shift 1] [--convert-to KEY | --convert-mu2 FILE.npy]
        [--out-format kaldi|numpy] [--compress] [--batch-size B] [--compute-dtype f32|bf16]

  z1       DIR/z1/: per utterance the (W, z1_dim) posterior means of z1, one row per window; with --shift 1 one row per frame,
           row f belonging to frame f of the input (the domain-invariant features of the FHVAE papers)
  mu2      DIR/mu2/: the closed-form mu2 of every utterance over its windows.  numpy: mu2.npy (U, z2_dim) + keys.txt; kaldi:
           a one-row matrix per key (feats.ark, feats.scp, len.scp), never compressed
  recon    DIR/recon/: per utterance (n, F) un-normalised features, every window decoded at its own z1 and z2 means and the
           overlapping windows averaged
  convert  DIR/convert/: the same with z2 replaced by --convert-to KEY's mu2 of this run, or by --convert-mu2 FILE.npy
           ((z2_dim,) for the corpus or (U, z2_dim), one row per utterance in feat-scp order)
  kaldi    feats.ark, feats.scp, len.scp (kaldi_io_lite.write_ark_scp / write_len_scp; --compress: Kaldi's automatic method,
           coded on the GPU by fhvae_kaldi_compress)            -> datasets.KaldiDataset
  numpy    <key>.npy, feats.scp, len.scp as prepare_numpy_data.py lays them out     -> datasets.NumpyDataset
Keys are in --feat-scp order and none is dropped: an utterance of one frame has one window.  summary.json holds the counts,
the shift, T and the compute dtype.  The checkpoint and the MVN statistics are loaded as eval_model.py loads them.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

WHAT = ("z1", "mu2", "recon", "convert")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Frame-level latents and reconstructed / converted features of a whole corpus")
    p.add_argument("--checkpoint", required=True)
    p.add_argument("--feat-scp", required=True)
    p.add_argument("--len-scp", required=True)
    p.add_argument("--data-format", default="numpy", choices=["numpy", "kaldi"], help="what --feat-scp points at")
    p.add_argument("--mvn-path", default=None)
    p.add_argument("--out", required=True, help="output directory (created)")
    p.add_argument("--what", nargs="+", required=True, choices=WHAT)
    p.add_argument("--shift", type=int, default=1, help="frames between window centres (1: one z1 row per frame)")
    tgt = p.add_mutually_exclusive_group()
    tgt.add_argument("--convert-to", default=None, metavar="KEY", help="convert: decode every utterance with this utterance's mu2")
    tgt.add_argument("--convert-mu2", default=None, metavar="FILE.npy", help="convert: a (z2_dim,) or (utterances, z2_dim) array")
    p.add_argument("--out-format", default="kaldi", choices=["kaldi", "numpy"])
    p.add_argument("--compress", action="store_true", help="kaldi output: compressed matrices (Kaldi's automatic method)")
    p.add_argument("--batch-size", type=int, default=16384, help="windows per forward")
    p.add_argument("--compute-dtype", default=None, choices=["f32", "bf16"], help="default: the checkpoint's")
    return p


def check_args(p: argparse.ArgumentParser, args, T: int):
    """What can only be checked once the checkpoint's T is known; errors are argparse errors."""
    if args.shift < 1:
        p.error("--shift %d must be at least 1" % args.shift)
    if args.batch_size < 1:
        p.error("--batch-size %d must be at least 1" % args.batch_size)
    limit = T - T // 2
    if args.shift > limit and any(w in args.what for w in ("recon", "convert")):
        p.error("--what recon / convert put overlapping windows back together: --shift %d leaves frames uncovered, it must be at most "
                "T - T // 2 = %d for the checkpoint's T = %d" % (args.shift, limit, T))
    if "convert" in args.what and args.convert_to is None and args.convert_mu2 is None:
        p.error("--what convert needs --convert-to KEY or --convert-mu2 FILE.npy")
    if args.compress and args.out_format != "kaldi":
        p.error("--compress codes Kaldi archives: use --out-format kaldi")


def write_archive(out_dir, keys, mats, out_format="kaldi", compress=False):
    """One matrix per key into `out_dir` (created): kaldi -> feats.ark + feats.scp + len.scp, numpy -> <key>.npy + feats.scp +
    len.scp.  mats: 2-D float arrays, or kaldi_io_lite.CompressedMatrix (kaldi only; written as they are).  compress: code
    the arrays on the host by Kaldi's automatic method.  Returns the number of entries."""
    import kaldi_io_lite as K

    os.makedirs(out_dir, exist_ok=True)
    keys = list(keys)
    if len(keys) != len(mats):
        raise ValueError("%d keys for %d matrices" % (len(keys), len(mats)))
    feat_scp, len_scp = os.path.join(out_dir, "feats.scp"), os.path.join(out_dir, "len.scp")
    if out_format == "kaldi":
        n = K.write_ark_scp(os.path.join(out_dir, "feats.ark"), feat_scp, zip(keys, mats), compress="auto" if compress else None)
    elif out_format == "numpy":
        with open(feat_scp, "w") as fh:
            for key, m in zip(keys, mats):
                path = os.path.join(out_dir, "%s.npy" % key)
                np.save(path, np.ascontiguousarray(m, dtype=np.float32))
                fh.write("%s %s\n" % (key, path))
        n = len(keys)
    else:
        raise ValueError("out_format %r: kaldi or numpy" % (out_format,))
    K.write_len_scp(len_scp, ((k, len(m)) for k, m in zip(keys, mats)))
    return n


def write_rows(out_dir, keys, rows, ptr, out_format, compress):
    """rows (N, X) on the device, utterance u its rows [ptr[u], ptr[u + 1]) -> write_archive; --compress codes on the device."""
    counts = np.diff(ptr)
    if out_format == "kaldi" and compress:
        import features

        mats = features.kaldi_compress(rows.contiguous(), counts, "auto", names=keys)
    else:
        host = rows.cpu().numpy()
        mats = [host[int(a):int(b)] for a, b in zip(ptr[:-1], ptr[1:])]
    return write_archive(out_dir, keys, mats, out_format, compress=False)


def main(argv=None) -> int:
    parser = build_parser()
    args = parser.parse_args(argv)
    import torch

    import utils

    model = utils.load_checkpoint_file(args.checkpoint, finetune=True)[0].eval()
    T = int(getattr(model, "seg_len", 20))
    check_args(parser, args, T)
    if args.compute_dtype is not None:
        if not hasattr(model, "compute_dtype"):
            parser.error("--compute-dtype: a %s checkpoint computes in f32 only" % model.model)
        model.compute_dtype = args.compute_dtype
    if not torch.cuda.is_available():
        print("extraction runs on a MI355X only (no CPU fallback)", file=sys.stderr)
        return 1
    import frames
    import hip_binding as hb

    dev = torch.device("cuda:0")
    model = model.to(dev)
    try:
        pool = frames.pool_from_scp(args.data_format, args.feat_scp, args.len_scp, args.mvn_path, T, args.shift, dev)
    except ValueError as e:
        print("extract_latents: %s" % e, file=sys.stderr)
        return 1
    keys, wrote = pool.keys, {}
    target = None
    if "convert" in args.what and args.convert_to is not None and args.convert_to not in keys:
        print("--convert-to %s: no such key in %s" % (args.convert_to, args.feat_scp), file=sys.stderr)
        return 1
    if "convert" in args.what and args.convert_mu2 is not None:
        target = torch.from_numpy(np.load(args.convert_mu2).astype(np.float32))
        if tuple(target.shape) not in ((model.z2_dim,), (pool.num_utts, model.z2_dim)):
            print("--convert-mu2: %s holds %s, not (%d,) or (%d, %d)" % (args.convert_mu2, tuple(target.shape), model.z2_dim,
                                                                        pool.num_utts, model.z2_dim), file=sys.stderr)
            return 1
    if any(w in args.what for w in ("z1", "mu2")) or (target is None and "convert" in args.what):
        z1, _, mu2 = frames.encode_frames(model, pool, args.batch_size)
        if "z1" in args.what:
            wrote["z1"] = write_rows(os.path.join(args.out, "z1"), keys, z1, pool.win_ptr_host, args.out_format, args.compress)
        if "mu2" in args.what:
            d = os.path.join(args.out, "mu2")
            rows = mu2.cpu().numpy()
            if args.out_format == "kaldi":
                wrote["mu2"] = write_archive(d, keys, [r[None, :] for r in rows], "kaldi")
            else:
                os.makedirs(d, exist_ok=True)
                np.save(os.path.join(d, "mu2.npy"), rows)
                with open(os.path.join(d, "keys.txt"), "w") as fh:
                    fh.writelines("%s\n" % k for k in keys)
                wrote["mu2"] = len(keys)
        if target is None and "convert" in args.what:
            target = mu2[keys.index(args.convert_to)]
        del z1
    for what, z2 in (("recon", None), ("convert", target)):
        if what in args.what:
            x = frames.convert_frames(model, pool, z2, args.batch_size)
            wrote[what] = write_rows(os.path.join(args.out, what), keys, x, pool.utt_ptr_host, args.out_format, args.compress)
            del x
    if hb.lstm_sync_status() != 0:
        print("a persistent recurrence launch gave up: the results are invalid", file=sys.stderr)
        return 3
    summary = {"checkpoint": os.path.basename(args.checkpoint), "utterances": pool.num_utts, "frames": pool.num_frames,
               "windows": pool.num_windows, "shift": args.shift, "T": T, "features": pool.F,
               "compute_dtype": getattr(model, "compute_dtype", "f32"), "out_format": args.out_format, "compress": bool(args.compress),
               "written": wrote}
    if "convert" in args.what:
        summary["convert_target"] = args.convert_to if args.convert_to is not None else os.path.basename(args.convert_mu2)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps(summary))
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main())
