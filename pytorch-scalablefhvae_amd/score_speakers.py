"""score_speakers.py -- speaker verification on embedding archives with the back end of spk_backend.py: train
centring / LDA / length normalisation / PLDA on one archive, score all pairs (and optionally a trial list) of another.  It works
on archives, so it needs no checkpoint: FHVAE mu2 from extract_latents.py --what mu2, or i-vectors / x-vectors from a Kaldi
archive as the papers' baseline.

    python score_speakers.py --train-emb DIR|SCP --eval-emb DIR|SCP (--utt2spk FILE | --spk-key-sep SEP)
        --backend cosine lda plda [--lda-dim K] [--no-length-norm] [--plda-iters 10] [--model FILE.npz] [--trials FILE]
        [--bins 4096] --out DIR
        [--snorm [--snorm-top 200] [--snorm-cohort DIR|SCP] [--snorm-cohort-mode speaker-means|rows] [--snorm-max-cohort N]]

An archive is a directory with mu2.npy + keys.txt (or ivectors.npy + keys.txt, what extract_ivectors.py writes), a directory with feats.scp (what extract_latents.py --out-format kaldi
writes: one-row matrices), or an scp file whose entries are one-row matrices or vectors.  --utt2spk / --spk-key-sep name the
speakers of both archives.  --trials lines are `<enrol-key> <test-key> target|nontarget` over the evaluation archive.

Writes speakers.json (per back end: eer, threshold, min_dcf, crossing_mass, n_target, n_nontarget, lo, hi; with --trials a
"trials" entry with the exact EER by sorting), hist_<backend>.npy, backend.npz (with lda or plda; --model reads one instead of
training) and, with --trials (which the PLDA scores), scores.txt (`<enrol-key> <test-key> <LLR>` per line).

--snorm scores every back end a second time, normalised against a cohort (score_norm.py): adaptive S-norm with the
--snorm-top largest cohort scores of either side (0: the whole cohort, S-norm).  The cohort is made from --snorm-cohort (default:
the training archive): its speakers' means, or its rows with --snorm-cohort-mode rows (an archive without speakers gives rows), at
most --snorm-max-cohort of them.  Per back end speakers.json gains a "snorm" block (the same figures plus "top" and "cohort"),
hist_<backend>_snorm.npy is written and, with --trials, scores_snorm.txt.  Without --snorm every output is what it was.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

BACKENDS = ("cosine", "lda", "plda")


def read_archive(path):
    """-> (keys, (S, D) float32 rows).  Errors name the key or the file."""
    import kaldi_io_lite as K

    if os.path.isdir(path):
        npy, txt, scp = (os.path.join(path, f) for f in ("mu2.npy", "keys.txt", "feats.scp"))
        if os.path.exists(npy) and os.path.exists(txt):
            rows = np.load(npy)
            with open(txt) as fh:
                keys = [line.strip() for line in fh if line.strip()]
            if rows.ndim != 2 or rows.shape[0] != len(keys):
                raise ValueError("%s: mu2.npy has shape %s, keys.txt %d keys" % (path, rows.shape, len(keys)))
            return _unique(path, keys), np.ascontiguousarray(rows, dtype=np.float32)
        ivec = os.path.join(path, "ivectors.npy")  # (what extract_ivectors.py writes)
        if os.path.exists(ivec) and os.path.exists(txt):
            rows = np.load(ivec)
            with open(txt) as fh:
                keys = [line.strip() for line in fh if line.strip()]
            if rows.ndim != 2 or rows.shape[0] != len(keys):
                raise ValueError("%s: ivectors.npy has shape %s, keys.txt %d keys" % (path, rows.shape, len(keys)))
            return _unique(path, keys), np.ascontiguousarray(rows, dtype=np.float32)
        if not os.path.exists(scp):
            raise ValueError("%s: neither mu2.npy + keys.txt nor feats.scp" % path)
        path = scp
    keys, rows = [], []
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            parts = line.split(None, 1)
            if not parts:
                continue
            if len(parts) != 2:
                raise ValueError("%s:%d: expected `<key> <file>[:offset]`, got %r" % (path, n, line.rstrip("\n")))
            key, spec = parts[0], parts[1].strip()
            try:
                m = K.load_mat(spec)
            except ValueError:
                m = K.load_vec(spec)
            m = np.asarray(m, dtype=np.float32)
            if m.ndim == 2 and m.shape[0] == 1:
                m = m[0]
            if m.ndim != 1 or m.shape[0] < 1:
                raise ValueError("%s:%d: key %r holds a matrix of shape %s, an embedding is one row" % (path, n, key, m.shape))
            if rows and m.shape[0] != rows[0].shape[0]:
                raise ValueError("%s:%d: key %r has %d columns, the entries before it %d" % (path, n, key, m.shape[0], rows[0].shape[0]))
            keys.append(key), rows.append(m)
    if not keys:
        raise ValueError("%s: no entry" % path)
    return _unique(path, keys), np.stack(rows)


def _unique(path, keys):
    seen = set()
    for k in keys:
        if k in seen:
            raise ValueError("%s: key %r is listed twice" % (path, k))
        seen.add(k)
    return keys


def read_trials(path, keys):
    """Lines `<enrol-key> <test-key> target|nontarget` -> ((n, 2) int32 rows of `keys`, (n,) bool target flags).  Errors name the line."""
    index = {k: i for i, k in enumerate(keys)}
    pairs, target = [], []
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != 3 or parts[2] not in ("target", "nontarget"):
                raise ValueError("%s:%d: expected `<enrol-key> <test-key> target|nontarget`, got %r" % (path, n, line.rstrip("\n")))
            for k in parts[:2]:
                if k not in index:
                    raise ValueError("%s:%d: key %r is not in the evaluation archive" % (path, n, k))
            pairs.append((index[parts[0]], index[parts[1]]))
            target.append(parts[2] == "target")
    if not pairs:
        raise ValueError("%s: no trial" % path)
    return np.asarray(pairs, dtype=np.int32), np.asarray(target, dtype=bool)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--train-emb", default=None, metavar="DIR|SCP", help="labelled embeddings the back end is trained on (lda, plda without --model)")
    p.add_argument("--eval-emb", required=True, metavar="DIR|SCP", help="the embeddings that are scored")
    spk = p.add_mutually_exclusive_group(required=True)
    spk.add_argument("--utt2spk", default=None, help="Kaldi utt2spk file naming each key's speaker, of both archives")
    spk.add_argument("--spk-key-sep", default=None, help="the speaker is the key up to the first SEP")
    p.add_argument("--backend", nargs="+", default=["cosine"], choices=BACKENDS)
    p.add_argument("--lda-dim", type=int, default=None, metavar="K", help="columns kept by the LDA (default: no LDA in front of the PLDA)")
    p.add_argument("--no-length-norm", action="store_true")
    p.add_argument("--plda-iters", type=int, default=10)
    p.add_argument("--model", default=None, metavar="FILE.npz", help="a backend.npz of an earlier run, instead of training")
    p.add_argument("--trials", default=None, metavar="FILE")
    p.add_argument("--bins", type=int, default=4096, help="score bins of the histograms (a power of two, 64..8192)")
    p.add_argument("--snorm", action="store_true", help="score a second time, normalised against a cohort (S-norm / AS-norm)")
    p.add_argument("--snorm-top", type=int, default=200, metavar="K", help="cohort scores kept per side (0: the whole cohort)")
    p.add_argument("--snorm-cohort", default=None, metavar="DIR|SCP", help="the cohort's embeddings (default: --train-emb)")
    p.add_argument("--snorm-cohort-mode", default="speaker-means", choices=("speaker-means", "rows"))
    p.add_argument("--snorm-max-cohort", type=int, default=None, metavar="N", help="at most N cohort rows (a random subset)")
    p.add_argument("--out", required=True)
    return p


def parse_args(argv=None) -> argparse.Namespace:
    p = build_parser()
    args = p.parse_args(argv)
    args.backend = [b for b in BACKENDS if b in args.backend]
    if args.bins < 64 or args.bins > 8192 or args.bins & (args.bins - 1):
        p.error("--bins %d must be a power of two in [64, 8192]" % args.bins)
    trained = [b for b in args.backend if b != "cosine"]
    if trained and args.train_emb is None and args.model is None:
        p.error("--backend %s needs --train-emb (or --model)" % " ".join(trained))
    if args.model is not None and args.train_emb is not None:
        p.error("--model replaces the training: leave --train-emb out")
    if args.plda_iters < 0:
        p.error("--plda-iters %d must not be negative" % args.plda_iters)
    if args.lda_dim is not None and args.lda_dim < 1:
        p.error("--lda-dim %d must be at least 1" % args.lda_dim)
    if "lda" in args.backend and args.model is None and args.lda_dim is None:
        p.error("--backend lda needs --lda-dim")
    if args.snorm:
        if args.snorm_cohort is None and args.train_emb is None:
            p.error("--snorm needs a cohort: --snorm-cohort (or --train-emb)")
        if args.snorm_top < 0:
            p.error("--snorm-top %d must not be negative" % args.snorm_top)
        if args.snorm_max_cohort is not None and args.snorm_max_cohort < 1:
            p.error("--snorm-max-cohort %d must be at least 1" % args.snorm_max_cohort)
    return args


def speakers_of(args, keys):
    import verification as V

    if args.utt2spk is not None:
        table = V.read_utt2spk(args.utt2spk)
        return [table.get(k) for k in keys]
    return V.speakers_from_keys(keys, args.spk_key_sep)


def read_cohort(args, dim):
    """The cohort rows of --snorm -> (Nc, dim) f32: the speakers' means of the cohort archive, or its rows (--snorm-cohort-mode
    rows, or an archive none of whose keys has a speaker)."""
    import score_norm as SN
    import verification as V

    path = args.snorm_cohort if args.snorm_cohort is not None else args.train_emb
    ckeys, cemb = read_archive(path)
    if cemb.shape[1] != dim:
        raise ValueError("the cohort %s has %d columns, %s has %d" % (path, cemb.shape[1], args.eval_emb, dim))
    speakers = speakers_of(args, ckeys)
    if args.snorm_cohort_mode == "rows" or all(s is None for s in speakers):
        return SN.make_cohort(cemb, None, "rows", args.snorm_max_cohort)
    return SN.make_cohort(cemb, V.labels_from_speakers(speakers)[0], "speaker-means", args.snorm_max_cohort)


def run(args) -> dict:
    import spk_backend as SB
    import verification as V

    keys, emb = read_archive(args.eval_emb)
    labels, n_spk = V.labels_from_speakers(speakers_of(args, keys))
    backend = None
    if any(b != "cosine" for b in args.backend):
        if args.model is not None:
            backend = SB.Backend.load(args.model)
        else:
            tkeys, temb = read_archive(args.train_emb)
            tlabels, _ = V.labels_from_speakers(speakers_of(args, tkeys))
            backend = SB.fit(temb, tlabels, args.lda_dim, not args.no_length_norm, args.plda_iters)
        if backend.dim != emb.shape[1]:
            raise ValueError("the back end was trained on %d columns, %s has %d" % (backend.dim, args.eval_emb, emb.shape[1]))
    trials = read_trials(args.trials, keys) if args.trials is not None else None
    os.makedirs(args.out, exist_ok=True)
    report = {"sequences": len(keys), "speakers": n_spk, "unlabelled": int((labels < 0).sum()), "bins": args.bins}
    columns, norm_columns = [], []
    cohort = read_cohort(args, emb.shape[1]) if args.snorm else None
    for name in args.backend:
        if name == "cosine":
            r = V.speaker_verification(emb, labels, n_bins=args.bins)
            hist = r.pop("hist")
            r = dict(SB.eer_from_hist(hist, -1.0, 1.0))
        else:
            r = backend.score_all_pairs(emb, labels, n_bins=args.bins, backend=name)
            hist = r.pop("hist")
        np.save(os.path.join(args.out, "hist_%s.npy" % name), hist)
        if trials is not None and name == "plda":
            s = backend.score_trials(emb, trials[0])
            columns.append(s)
            t = SB.exact_eer(s, trials[1])
            r["trials"] = {"eer": t["eer"], "threshold": t["threshold"], "n_target": t["n_target"], "n_nontarget": t["n_nontarget"]}
        if cohort is not None:
            import score_norm as SN

            rn = SN.score_all_pairs(backend, emb, labels, cohort, top=args.snorm_top, which=name, n_bins=args.bins)
            np.save(os.path.join(args.out, "hist_%s_snorm.npy" % name), rn.pop("hist"))
            if trials is not None and name == "plda":
                s = SN.score_trials(backend, emb, trials[0], cohort, top=args.snorm_top, which=name)
                norm_columns.append(s)
                t = SB.exact_eer(s, trials[1])
                rn["trials"] = {"eer": t["eer"], "threshold": t["threshold"], "n_target": t["n_target"], "n_nontarget": t["n_nontarget"]}
            r["snorm"] = rn
        report[name] = r
    if backend is not None:
        backend.save(os.path.join(args.out, "backend.npz"))
    if trials is not None and columns:
        with open(os.path.join(args.out, "scores.txt"), "w") as fh:
            for (i, j), s in zip(trials[0], columns[0]):
                fh.write("%s %s %.9g\n" % (keys[int(i)], keys[int(j)], float(s)))
    if trials is not None and norm_columns:
        with open(os.path.join(args.out, "scores_snorm.txt"), "w") as fh:
            for (i, j), s in zip(trials[0], norm_columns[0]):
                fh.write("%s %s %.9g\n" % (keys[int(i)], keys[int(j)], float(s)))
    with open(os.path.join(args.out, "speakers.json"), "w") as fh:
        json.dump(report, fh, indent=1)
    return report


def main(argv=None) -> int:
    args = parse_args(argv)
    if args.trials is not None and "plda" not in args.backend:
        print("--trials are scored by the PLDA: add plda to --backend", file=sys.stderr)
        return 1
    try:
        report = run(args)
    except (ValueError, OSError) as e:
        print("score_speakers: %s" % e, file=sys.stderr)
        return 1
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main())
