"""prepare_kaldi_data.py -- audio files (WAV, FLAC or SPHERE) listed in wav.scp -> Kaldi filterbank features in the Kaldi layout the loaders read
(the reference's prepare_kaldi_data.py:10-136, with compute-fbank-feats and feat-to-len replaced by
features.compute_kaldi_fbank on the MI355X and kaldi_io_lite; no Kaldi binary is run).

    python pytorch-scalablefhvae_amd/prepare_kaldi_data.py DATASET_DIR [--fbank_conf ./misc/fbank.conf] [--set_name train]
        [--seed 0] [--resample] [--compress [--compression-method auto]] [--verify-md5] [--vad {mark,drop} [--vad_conf FILE]]
        [--mfcc_conf FILE] [--add-deltas [--delta-order 2] [--delta-window 2]]
        [--cmvn-sliding [--cmn-window 300] [--cmn-min-window 100] [--no-cmn-center] [--cmn-norm-vars]]

For every set (train, dev and test in turn unless --set_name is given) it reads <DATASET_DIR>/<set>/wav.scp ("<key> <path>"
lines) and writes, in wav.scp order, <DATASET_DIR>/<set>/feats.ark (binary archive of float32 matrices), feats.scp
("<key> <feats.ark>:<offset>") and len.scp ("<key> <nframes>").  With --compress the archive holds Kaldi compressed
matrices (what copy-feats --compress=true writes, about a quarter of the size): the features are coded on the GPU and only
the bytes are downloaded; --compression-method picks Kaldi's automatic method (default), "two-byte" or "one-byte".  --fbank_conf is a Kaldi config file the user supplies,
one option per line, for example

    --window-type=hamming
    --sample-frequency=16000
    --dither=1
    --num-mel-bins=80

(features.kaldi_fbank_options lists what is supported).

With --vad the frames are marked voiced or not as compute-vad-decision does (features.kaldi_energy_vad: Kaldi's raw log energy
of the fbank's own frames, no dither; --vad_conf is a config file of the four --vad-* options, features.kaldi_vad_options), on
the GPU from the waveform the features are computed from.  Both modes write the decisions of every utterance over its
ORIGINAL frames as float vectors (1.0 / 0.0) to <DATASET_DIR>/<set>/vad.ark and vad.scp.  "mark" leaves feats.ark, feats.scp
and len.scp what a run without the flag writes; "drop" keeps the voiced rows only (select-voiced-frames: selected on the GPU
in front of the compression and the download; len.scp then holds the voiced count), skips an utterance without a voiced
frame, naming it on stderr, and closes with one line that counts the skipped utterances and the share of frames dropped.

With --mfcc_conf FILE the archive holds MFCCs instead (compute-mfcc-feats: kaldi_post.kaldi_mfcc_options lists what the file
may hold; --fbank_conf is not read then).  --add-deltas appends delta and delta-delta features (add-deltas) and --cmvn-sliding
subtracts the mean of a sliding window (apply-cmvn-sliding --center=true --cmn-window=300 unless --no-cmn-center /
--cmn-window say otherwise; --cmn-norm-vars also divides by the window's standard deviation); both are valid with either
configuration and are applied on the GPU in the order of Kaldi's recipes: deltas, CMVN, then --vad drop's row selection, then
--compress.  Without these flags nothing changes.

Differences from the reference:
  * --kaldi_root is accepted and ignored.
  * dither noise comes from a counter-based generator keyed by --seed and zlib.crc32 of the utterance key, so a file's
    features are reproducible and do not depend on its place in wav.scp (Kaldi's rand() stream is neither).
  * only plain "<key> <path>" entries: a line ending in "|" (a Kaldi pipe) is refused.  The files are read by
    features.read_audio_batch: integer PCM WAV, native FLAC (decoded on the GPU; --verify-md5 also checks the decoded audio
    against the MD5 in each file) and uncompressed NIST SPHERE, so a LibriSpeech or TIMIT wav.scp needs no sox / sph2pipe pipe.
  * a multi-channel file contributes channel 0, as Kaldi reads it (prepare_numpy_data.py averages the channels).
  * a file whose rate differs from sample-frequency is an error, as in Kaldi, unless --resample converts it on the GPU
    (features.resample); a file shorter than one frame is an error that names it (Kaldi skips it with a warning).
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import os
import sys
import time
from pathlib import Path

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import features  # noqa: E402
import kaldi_io_lite  # noqa: E402

READ_THREADS = 8  # file reads overlapping the GPU work (of the 16 CPUs a job gets; not sized by os.cpu_count())
CHUNK_FILES = 512  # files read ahead of the batch being computed
VAD_MODES = (None, "mark", "drop")


def read_wav_scp(path):
    entries = []
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            if not line.strip():
                continue
            parts = line.rstrip().split(None, 1)
            if len(parts) != 2:
                raise ValueError("%s:%d: expected \"<key> <path>\"" % (path, ln))
            if parts[1].endswith("|"):
                raise ValueError("%s:%d: %s is a piped entry (\"... |\"); only plain WAV paths are supported: run the command "
                                 "and list its output file" % (path, ln, parts[0]))
            entries.append((parts[0], parts[1]))
    return entries


def prepare_kaldi(dataset_dir, set_name, fbank_conf="./misc/fbank.conf", kaldi_root=None, seed=0, resample=False, timings=None,
                  compress=None, verify_md5=False, vad=None, vad_conf=None, mfcc_conf=None, deltas=None, cmvn=None):
    """prepare_kaldi_data.py:10-82: features of every sequence of <dataset_dir>/<set_name>/wav.scp.
    Returns (count, (dataset_dir, feats.ark, feats.scp, len.scp)).  `timings` (optional dict) receives seconds spent in
    "read", "gpu" and "write".  `compress`: None (float32 matrices) or a method of kaldi_io_lite.METHODS.  `vad`: None, "mark"
    or "drop" (the module docstring) with `vad_conf`, what features.kaldi_vad_options takes; then the result's second entry
    also holds vad.ark and vad.scp, and `count` counts the utterances written.  `mfcc_conf` (what kaldi_post.kaldi_mfcc_options
    takes): MFCCs instead of fbank features, `fbank_conf` is not read; `deltas` / `cmvn` (kaldi_post.deltas_spec / cmvn_spec):
    the two steps behind the features on the device.  With all three None the path is features.compute_kaldi_fbank's, as before."""
    if vad not in VAD_MODES:
        raise ValueError("vad must be one of %s, got %r" % (", ".join(str(m) for m in VAD_MODES), vad))
    if vad is None and vad_conf is not None:
        raise ValueError("--vad_conf needs --vad {mark,drop}")
    post = mfcc_conf is not None or deltas is not None or cmvn is not None
    if post:
        import kaldi_post

        opts = kaldi_post.kaldi_mfcc_options(mfcc_conf) if mfcc_conf is not None else features.kaldi_fbank_options(fbank_conf)
    else:
        opts = features.kaldi_fbank_options(fbank_conf)
    conf_name = mfcc_conf if mfcc_conf is not None else fbank_conf
    vad_opts = features.kaldi_vad_options(vad_conf) if vad is not None else None
    sr = int(opts["sample-frequency"])
    set_dir = Path(dataset_dir) / set_name
    wav_path = set_dir / "wav.scp"
    if not os.path.exists(wav_path):
        raise ValueError(f"The wav.scp file at {wav_path} does not exist!")
    feat_ark, feat_scp, len_scp = set_dir / "feats.ark", set_dir / "feats.scp", set_dir / "len.scp"
    vad_ark, vad_scp = set_dir / "vad.ark", set_dir / "vad.scp"
    decisions = []  # (key, float vector) of every utterance, in wav.scp order (one byte per 10 ms of audio)
    stats = {"skipped": 0, "in": 0, "out": 0}
    entries = read_wav_scp(wav_path)
    t = {} if timings is None else timings
    for k in ("read", "gpu", "write"):
        t.setdefault(k, 0.0)
    start_time = time.time()
    lens = []

    def load(chunk):
        got = features.read_audio_batch([path for _, path in chunk], channel=0, verify_md5=verify_md5, threads=READ_THREADS)
        return [(key, path, y, rate) for (key, path), (y, rate) in zip(chunk, got)]

    def items():
        chunks = [entries[i:i + CHUNK_FILES] for i in range(0, len(entries), CHUNK_FILES)]
        with cf.ThreadPoolExecutor(max_workers=1) as pool:
            pending = pool.submit(load, chunks[0]) if chunks else None
            for ci in range(len(chunks)):
                t0 = time.time()
                got = pending.result()
                t["read"] += time.time() - t0
                # the next chunk's files are read (and its FLAC files decoded) while this one is on the GPU and being written
                pending = pool.submit(load, chunks[ci + 1]) if ci + 1 < len(chunks) else None
                if not resample:
                    for key, path, _, rate in got:
                        if rate != sr:
                            raise ValueError(f"{key} ({path}): sample rate {rate} differs from sample-frequency {sr} of "
                                             f"{conf_name} (convert the file or pass --resample)")
                t0 = time.time()
                more = {} if vad is None else {"vad": {"opts": vad_opts, "drop": vad == "drop"}}
                if post:
                    more.update(kind="mfcc" if mfcc_conf is not None else "fbank", deltas=deltas, cmvn=cmvn)
                feats = (kaldi_post.compute_kaldi_feats if post else features.compute_kaldi_fbank)(
                    [g[2] for g in got], opts, seed=seed, stream_ids=[features.kaldi_stream_id(g[0]) for g in got],
                    names=["%s (%s)" % (g[0], g[1]) for g in got], rates=[g[3] for g in got] if resample else None,
                    compress=compress, **more)
                feats, vads = feats if vad is not None else (feats, [None] * len(got))
                dt = time.time() - t0
                t["gpu"] += dt
                t0 = time.time()
                for g, feat, v in zip(got, feats, vads):
                    if v is not None:
                        decisions.append((g[0], v.astype("float32")))
                        stats["in"] += len(v)
                        stats["out"] += len(feat)
                        if vad == "drop" and len(feat) == 0:
                            print(f"prepare_kaldi_data: {g[0]} ({g[1]}) has no voiced frame: skipped", file=sys.stderr)
                            stats["skipped"] += 1
                            continue
                    lens.append((g[0], len(feat)))
                    yield g[0], feat
                    if len(lens) % 1000 == 0:
                        print(f"{len(lens)} {set_name} files in {time.time() - start_time} seconds.")
                t["write"] += time.time() - t0

    count = kaldi_io_lite.write_ark_scp(str(feat_ark), str(feat_scp), items())
    kaldi_io_lite.write_len_scp(len_scp, lens)
    print(f"Processed {count} files in {set_name} set over {time.time() - start_time} seconds.")
    if vad is not None:
        kaldi_io_lite.write_vec_ark_scp(str(vad_ark), str(vad_scp), decisions)
    if vad == "drop":
        print("Skipped %d of %d utterances without a voiced frame; dropped %d of %d frames (%.1f%%) in the %s set."
              % (stats["skipped"], count + stats["skipped"], stats["in"] - stats["out"], stats["in"],
                 100.0 * (stats["in"] - stats["out"]) / max(stats["in"], 1), set_name))
    if vad is not None:
        return count, (Path(dataset_dir), feat_ark, feat_scp, len_scp, vad_ark, vad_scp)
    return count, (Path(dataset_dir), feat_ark, feat_scp, len_scp)


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("dataset_dir", type=str, help="Directory containing subdirectories with wav.scp files")
    p.add_argument("--fbank_conf", type=str, default="./misc/fbank.conf", help="Kaldi fbank configuration")
    p.add_argument("--kaldi_root", type=str, default=None, help="Kaldi root directory (ignored: no Kaldi binary is run)")
    p.add_argument("--set_name", type=str, default=None, help="Set {train, dev, test} to operate on. Leave blank for all three")
    p.add_argument("--seed", type=int, default=0, help="Seed of the dither noise")
    p.add_argument("--resample", action="store_true",
                   help="Convert files whose rate differs from the configuration's sample-frequency on the GPU")
    p.add_argument("--verify-md5", action="store_true", help="Check every FLAC file's decoded audio against the MD5 it carries")
    p.add_argument("--compress", action="store_true", help="Write Kaldi compressed matrices (coded on the GPU), as copy-feats --compress=true does")
    p.add_argument("--compression-method", type=str, default="auto", choices=list(kaldi_io_lite.METHODS),
                   help="With --compress: Kaldi's automatic method (one byte with column headers; two bytes up to 8 frames), or two or one byte per value")
    p.add_argument("--vad", type=str, default=None, choices=["mark", "drop"],
                   help="Energy VAD on the GPU (compute-vad-decision): write vad.ark / vad.scp (mark), or also keep the voiced frames only (drop, select-voiced-frames)")
    p.add_argument("--vad_conf", type=str, default=None,
                   help="With --vad: Kaldi config file of --vad-energy-threshold, --vad-energy-mean-scale, --vad-frames-context, --vad-proportion-threshold")
    p.add_argument("--mfcc_conf", type=str, default=None,
                   help="Kaldi MFCC configuration (compute-mfcc-feats): write MFCCs instead of fbank features; --fbank_conf is not read")
    add_post_arguments(p)
    return p


def add_post_arguments(p):
    """The --add-deltas / --cmvn-sliding arguments (shared with postprocess_kaldi_feats.py); post_specs reads them."""
    p.add_argument("--add-deltas", action="store_true", help="Append delta features on the GPU (add-deltas)")
    p.add_argument("--delta-order", type=int, default=None, help="With --add-deltas: 1 or 2 (default 2)")
    p.add_argument("--delta-window", type=int, default=None, help="With --add-deltas: the window of one differentiation, 1 to 8 (default 2)")
    p.add_argument("--cmvn-sliding", action="store_true", help="Sliding-window mean normalisation on the GPU (apply-cmvn-sliding)")
    p.add_argument("--cmn-window", type=int, default=None, help="With --cmvn-sliding: frames in the window (default 300)")
    p.add_argument("--cmn-min-window", type=int, default=None, help="With --cmvn-sliding --no-cmn-center: the least window at an utterance's start (default 100)")
    p.add_argument("--no-cmn-center", action="store_true", help="With --cmvn-sliding: the window ends at the frame instead of being centred on it")
    p.add_argument("--cmn-norm-vars", action="store_true", help="With --cmvn-sliding: also normalise the variance over the window")


#: the arguments of the steps of kaldi_post.py; at their defaults main() prints the argument list without them, as it was
POST_ARGS = ("mfcc_conf", "add_deltas", "delta_order", "delta_window", "cmvn_sliding", "cmn_window", "cmn_min_window", "no_cmn_center",
             "cmn_norm_vars")


def post_specs(parser, args):
    """The --add-deltas / --cmvn-sliding arguments (shared with postprocess_kaldi_feats.py) -> (deltas_spec, cmvn_spec), None
    for a step not asked for; contradictory arguments end in parser.error before any work."""
    if not args.add_deltas and (args.delta_order is not None or args.delta_window is not None):
        parser.error("--delta-order / --delta-window need --add-deltas")
    if not args.cmvn_sliding and (args.cmn_window is not None or args.cmn_min_window is not None or args.no_cmn_center or args.cmn_norm_vars):
        parser.error("--cmn-window / --cmn-min-window / --no-cmn-center / --cmn-norm-vars need --cmvn-sliding")
    if not (args.add_deltas or args.cmvn_sliding):
        return None, None
    import kaldi_post

    try:
        deltas = kaldi_post.deltas_spec(2 if args.delta_order is None else args.delta_order,
                                        2 if args.delta_window is None else args.delta_window) if args.add_deltas else None
        cmvn = kaldi_post.cmvn_spec(300 if args.cmn_window is None else args.cmn_window,
                                    100 if args.cmn_min_window is None else args.cmn_min_window, not args.no_cmn_center,
                                    args.cmn_norm_vars) if args.cmvn_sliding else None
    except ValueError as e:
        parser.error(str(e))
    return deltas, cmvn


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.vad_conf is not None and args.vad is None:
        parser.error("--vad_conf needs --vad {mark,drop}")
    if args.mfcc_conf is not None and args.fbank_conf != parser.get_default("fbank_conf"):
        parser.error("--mfcc_conf and --fbank_conf exclude each other")
    deltas, cmvn = post_specs(parser, args)
    print(argparse.Namespace(**{k: v for k, v in vars(args).items() if k not in POST_ARGS or v not in (None, False)}))
    if args.kaldi_root is not None:
        print("--kaldi_root is ignored: the features are computed on the GPU, no Kaldi binary is run")
    sets = ["train", "dev", "test"] if args.set_name is None else [args.set_name]
    t0 = time.time()
    total = 0
    try:
        for s in sets:
            total += prepare_kaldi(args.dataset_dir, s, args.fbank_conf, args.kaldi_root, args.seed, args.resample,
                                   compress=args.compression_method if args.compress else None, verify_md5=args.verify_md5,
                                   vad=args.vad, vad_conf=args.vad_conf, mfcc_conf=args.mfcc_conf, deltas=deltas, cmvn=cmvn)[0]
    except ValueError as e:
        print("prepare_kaldi_data: %s" % e, file=sys.stderr)
        return 1
    if len(sets) > 1:
        print(f"Processed {total} files in {time.time() - t0} seconds.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
