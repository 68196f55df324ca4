"""extract_ivectors.py -- i-vectors for a whole corpus (ivector.py does the work): the speaker baseline of the FHVAE
papers, from this project's own features and UBM.  With prepare_kaldi_data.py --mfcc_conf in front and score_speakers.py behind,

    prepare_kaldi_data.py --mfcc_conf ... -> fit_gmm.py --on feats -> extract_ivectors.py -> score_speakers.py --backend cosine lda plda

runs with nothing from outside.

    python pytorch-scalablefhvae_amd/extract_ivectors.py --feat-scp S --len-scp S [--data-format numpy|kaldi] [--mvn-path P]
        [--train-feat-scp S --train-len-scp S]
        (--ubm FILE.npz | --ubm-k K [--ubm-iters 50] [--seed 0])
        (--rank R [--iters 10] [--no-min-div] | --model FILE.npz)
        --out DIR [--out-format numpy|kaldi]

  --ubm FILE       the gmm.npz of fit_gmm.py --on feats on rows of the same kind;  --ubm-k K fits one here (gmm.fit) on the
                   training rows
  --rank R         fit the total-variability matrix (ivector.fit) on the training archive: --train-feat-scp / --train-len-scp, or
                   the archive that is extracted when they are left out
  --model FILE     apply the ivector.npz of an earlier run; on the archive it came from it reproduces ivectors.npy byte for byte

It writes under --out: ivectors.npy (utterances, R) float64 + keys.txt, or with --out-format kaldi feats.scp / len.scp of one-row
matrices (extract_latents.write_rows) -- either is an archive score_speakers.py reads; ivector.npz (ivector.save) and ubm.npz
(gmm.save); ivector.json: rank, C, width, utterances, frames, Q (after the start and every step; empty with --model), steps,
not_pd (utterances whose posterior precision did not factor: their rows are NaN), seed.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="i-vector extraction on the GPU: per-utterance statistics under a UBM, EM for the total-variability matrix")
    p.add_argument("--feat-scp", required=True)
    p.add_argument("--len-scp", required=True)
    p.add_argument("--data-format", default="numpy", choices=["numpy", "kaldi"], help="what the scp files point at")
    p.add_argument("--mvn-path", default=None)
    p.add_argument("--train-feat-scp", default=None, help="the archive the UBM (--ubm-k) and the extractor (--rank) are fitted on")
    p.add_argument("--train-len-scp", default=None)
    ubm = p.add_mutually_exclusive_group(required=True)
    ubm.add_argument("--ubm", default=None, metavar="FILE.npz", help="a gmm.npz of fit_gmm.py --on feats")
    ubm.add_argument("--ubm-k", type=int, default=None, metavar="K", help="fit a UBM of K components here")
    p.add_argument("--ubm-iters", type=int, default=50)
    p.add_argument("--seed", type=int, default=0)
    how = p.add_mutually_exclusive_group(required=True)
    how.add_argument("--rank", type=int, default=None, metavar="R", help="fit an extractor of this rank")
    how.add_argument("--model", default=None, metavar="FILE.npz", help="apply this ivector.npz instead of fitting one")
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--no-min-div", action="store_true")
    p.add_argument("--out", required=True, help="output directory (created)")
    p.add_argument("--out-format", default="numpy", choices=["numpy", "kaldi"])
    return p


def parse_args(argv=None):
    import ivector

    p = build_parser()
    args = p.parse_args(argv)
    if (args.train_feat_scp is None) != (args.train_len_scp is None):
        p.error("--train-feat-scp and --train-len-scp come together")
    if args.rank is not None and not 1 <= args.rank <= ivector.IV_MAX_RANK:
        p.error("--rank %d must lie in [1, %d]" % (args.rank, ivector.IV_MAX_RANK))
    if args.ubm_k is not None and args.ubm_k < 1:
        p.error("--ubm-k %d must be at least 1" % args.ubm_k)
    if args.iters < 1 or args.ubm_iters < 1:
        p.error("--iters and --ubm-iters must be at least 1")
    if args.seed < 0 or args.seed >= 2 ** 32:
        p.error("--seed %d must lie in [0, 2^32)" % args.seed)
    if args.model is not None and args.train_feat_scp is not None and args.ubm_k is None:
        p.error("--model and --ubm replace the training: leave --train-feat-scp out")
    return args


def gpu_available() -> bool:
    import torch

    return torch.cuda.is_available()


def corpus(args, feat_scp, len_scp):
    """-> (keys, rows (N, D) f32 on the device, ptr (U + 1,) int64 numpy) of an archive: the normalised input, as fit_gmm.py --on feats."""
    import torch

    import frames

    pool = frames.pool_from_scp(args.data_format, feat_scp, len_scp, args.mvn_path, 20, 1, torch.device("cuda:0"))
    rows = frames.corpus_rows(None, pool, "feats", "i-vector extraction").contiguous()
    if not bool(torch.isfinite(rows).all()):
        raise ValueError("%s holds values that are not finite" % feat_scp)
    return list(pool.keys), rows, np.asarray(pool.utt_ptr_host, dtype=np.int64)


def run(args) -> dict:
    import extract_latents
    import gmm
    import ivector

    keys, rows, ptr = corpus(args, args.feat_scp, args.len_scp)
    width = int(rows.shape[1])
    if width > ivector.IV_MAX_DP:
        raise ValueError("%s has %d values per frame, the mixture kernels take at most %d" % (args.feat_scp, width, ivector.IV_MAX_DP))
    train = None
    if args.train_feat_scp is not None:
        train = corpus(args, args.train_feat_scp, args.train_len_scp)
        if int(train[1].shape[1]) != width:
            raise ValueError("%s has %d values per frame, %s has %d" % (args.train_feat_scp, int(train[1].shape[1]), args.feat_scp, width))
    tkeys, trows, tptr = train if train is not None else (keys, rows, ptr)
    if args.ubm is not None:
        ubm = gmm.load(args.ubm)
    else:
        ubm, _ = gmm.fit(trows, args.ubm_k, iters=args.ubm_iters, seed=args.seed)
    ubm = {key: np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float64) for key, v in ubm.items()}
    if ubm["means"].shape[1] != width:
        raise ValueError("the UBM is %s, but %s has %d values per frame" % (ubm["means"].shape, args.feat_scp, width))
    n, f = ivector.utterance_stats(rows, ptr, ubm)
    hist = {"Q": [], "steps": []}
    if args.model is not None:
        model = ivector.load(args.model)
        if model["means"].shape != ubm["means"].shape or not np.array_equal(model["means"], ubm["means"]) or not np.array_equal(model["variances"], ubm["variances"]):
            raise ValueError("%s was not fitted under this UBM (its means and variances differ)" % args.model)
    else:
        tn, tf = (n, f) if train is None else ivector.utterance_stats(trows, tptr, ubm)
        model, hist = ivector.fit(tn, tf, ubm, args.rank, iters=args.iters, seed=args.seed, min_div=not args.no_min_div)
        # through the file's own form (numpy float64), so that --model with ivector.npz repeats this run bit for bit
        model = {key: np.ascontiguousarray(v, dtype=np.float64) for key, v in model.items()}
    w, bad = ivector.extract(n, f, model, with_bad=True)
    info = {"rank": int(model["T"].shape[1]), "C": int(ubm["means"].shape[0]), "width": width, "utterances": len(keys), "frames": int(ptr[-1]),
            "Q": [float(q) for q in hist["Q"]], "steps": list(hist["steps"]), "not_pd": int(bad), "seed": int(args.seed)}
    os.makedirs(args.out, exist_ok=True)
    if args.out_format == "numpy":
        np.save(os.path.join(args.out, "ivectors.npy"), np.ascontiguousarray(w.cpu().numpy(), dtype=np.float64))
        with open(os.path.join(args.out, "keys.txt"), "w") as fh:
            fh.write("".join("%s\n" % k for k in keys))
    else:
        extract_latents.write_rows(args.out, keys, w.float(), np.arange(len(keys) + 1, dtype=np.int64), "kaldi", False)
    ivector.save(os.path.join(args.out, "ivector.npz"), model)
    gmm.save(os.path.join(args.out, "ubm.npz"), ubm)
    with open(os.path.join(args.out, "ivector.json"), "w") as fh:
        json.dump(info, fh, indent=1)
    return info


def main(argv=None) -> int:
    args = parse_args(argv)
    if not gpu_available():
        print("the mixture runs on a MI355X only (no CPU fallback)", file=sys.stderr)
        return 1
    try:
        info = run(args)
    except (ValueError, OSError, RuntimeError) as e:
        print("extract_ivectors: %s" % e, file=sys.stderr)
        return 1
    print(json.dumps(info))
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main())
