"""prepare_numpy_data.py -- audio files (WAV, FLAC or SPHERE) listed in wav.scp -> the numpy feature layout the loaders read (the reference's
prepare_numpy_data.py:50-205, with the features computed on the MI355X by features.compute_features).

    python pytorch-scalablefhvae_amd/prepare_numpy_data.py DATASET_DIR [--np_dir OUT] [--set_name train]
        [--ftype {fbank,spec}] [--sr RATE] [--resample] [--win_t 0.025] [--hop_t 0.010] [--n_mels 80] [--verify-md5]
        [--vad {mark,drop} [--vad_th_ratio 0.52]]

For every set (train, dev and test in turn unless --set_name is given) it reads <DATASET_DIR>/<set>/wav.scp ("<seq> <path>"
lines) and writes, in wav.scp order, <OUT>/<set>/<seq>.npy (float32, (nframes, n_mels) or (nframes, n_fft // 2 + 1)) plus
<OUT>/<set>/feats.scp ("<seq> <path.npy>") and <OUT>/<set>/len.scp ("<seq> <nframes>"); OUT is --np_dir or DATASET_DIR.

With --vad the reference's AudioUtils.energy_vad (utils.py:275-300; features.energy_vad, th_ratio = --vad_th_ratio) decides for
every frame whether it is voiced, on the GPU from the waveform the features are computed from.  Both modes write the
decisions of every sequence over its ORIGINAL frames: <OUT>/<set>/<seq>.vad.npy (uint8 0 / 1, (nframes,)) plus vad.scp
("<seq> <path.vad.npy>").  "mark" leaves the features, feats.scp and len.scp what a run without the flag writes; "drop" keeps
the voiced rows only (selected on the GPU in front of the download; len.scp then holds the voiced count), skips a sequence
without a voiced frame, naming it on stderr, and closes with one line that counts the skipped sequences and the share of
frames dropped, as Kaldi's select-voiced-frames does.

Differences from the reference:
  * wav.scp is read from DATASET_DIR even when --np_dir is given (the reference looks for it under the output directory,
    prepare_numpy_data.py:81-92, which only works when both are the same).
  * resampling is opt-in: by default every file of a set must have one sample rate, and a --sr that differs from a
    file's rate is an error.  With --resample (which needs --sr, the target rate) files at other rates are converted to
    --sr on the GPU as the reference's librosa.load does (resampy kaiser_best; features.resample); files already at --sr
    go through unchanged.  The reference always resampled.
  * files are read by features.read_audio_batch: integer PCM WAV, native FLAC (decoded on the GPU, a chunk of files per
    launch; --verify-md5 also checks the decoded audio against the MD5 in each file) and uncompressed NIST SPHERE, told
    apart by their first bytes; sets run one after the other on the GPU instead of a pool of 3 processes.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import contextlib
import os
import sys
import time
from pathlib import Path

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import numpy as np  # noqa: E402

import features  # noqa: E402

READ_THREADS = 8  # file reads overlapping the GPU work (of the 16 CPUs a job gets; not sized by os.cpu_count())
CHUNK_FILES = 512  # files read ahead of the batch being computed
VAD_MODES = (None, "mark", "drop")


def read_wav_scp(path):
    with open(path) as fh:
        return [tuple(line.rstrip().split(None, 1)) for line in fh if line.strip()]


def prepare_numpy(dataset, set_name, dataset_dir, output_dir=None, ftype="fbank", sample_rate=None, win_t=0.025, hop_t=0.010,
                  n_mels=80, timings=None, resample=False, verify_md5=False, vad=None, vad_th_ratio=features.VAD_TH_RATIO):
    """prepare_numpy_data.py:50-129: features of every sequence of <dataset_dir>/<set_name>/wav.scp.
    Returns (count, (wav_path, feat_path, len_path)).  `timings` (optional dict) receives seconds spent in "read", "gpu"
    and "write".  `resample`: files whose rate differs from `sample_rate` (required then) are converted to it on the GPU.
    `vad`: None, "mark" or "drop" (the module docstring); then the result's third entry is
    (wav_path, feat_path, len_path, vad_path) and `count` counts the sequences written."""
    if vad not in VAD_MODES:
        raise ValueError("vad must be one of %s, got %r" % (", ".join(str(m) for m in VAD_MODES), vad))
    if resample and sample_rate is None:
        raise ValueError("--resample needs --sr, the target sample rate")
    wav_path = Path(dataset_dir) / set_name / "wav.scp"
    set_path = Path(output_dir if output_dir is not None else dataset_dir) / set_name
    if not os.path.exists(wav_path):
        raise ValueError(f"The wav.scp file at {wav_path} does not exist!")
    os.makedirs(set_path, exist_ok=True)
    feat_path, len_path, vad_path = set_path / "feats.scp", set_path / "len.scp", set_path / "vad.scp"
    skipped = frames_in = frames_out = 0
    entries = read_wav_scp(wav_path)
    t = {"read": 0.0, "gpu": 0.0, "write": 0.0} if timings is None else timings
    for k in ("read", "gpu", "write"):
        t.setdefault(k, 0.0)
    start_time = time.time()
    count = 0

    def load(chunk):
        got = features.read_audio_batch([path for _, path in chunk], verify_md5=verify_md5, threads=READ_THREADS)
        return [(seq, path, y, sr) for (seq, path), (y, sr) in zip(chunk, got)]

    chunks = [entries[i:i + CHUNK_FILES] for i in range(0, len(entries), CHUNK_FILES)]
    with cf.ThreadPoolExecutor(max_workers=1) as pool, open(feat_path, "w") as featfile, open(len_path, "w") as lenfile, \
            (open(vad_path, "w") if vad is not None else contextlib.nullcontext()) as vadfile:
        pending = pool.submit(load, chunks[0]) if chunks else None
        for ci in range(len(chunks)):
            t0 = time.time()
            got = pending.result()
            t["read"] += time.time() - t0
            # the next chunk's files are read (and its FLAC files decoded) while this one is on the GPU and being written
            pending = pool.submit(load, chunks[ci + 1]) if ci + 1 < len(chunks) else None
            for seq, path, _, sr in got:
                if resample:
                    continue
                if sample_rate is None:
                    sample_rate = sr
                elif sr != sample_rate:
                    raise ValueError(f"{path}: sample rate {sr} differs from {sample_rate} (no resampling: convert the file "
                                     f"or pass the matching --sr)")
            t0 = time.time()
            feats = features.compute_features([g[2] for g in got], sample_rate, ftype, win_t, hop_t, n_mels,
                                              names=["%s (%s)" % (g[0], g[1]) for g in got],
                                              rates=[g[3] for g in got] if resample else None,
                                              **({} if vad is None else {"vad": {"th_ratio": vad_th_ratio, "drop": vad == "drop"}}))
            feats, vads = feats if vad is not None else (feats, [None] * len(got))
            t["gpu"] += time.time() - t0
            t0 = time.time()
            for (seq, path, _, _), feat, v in zip(got, feats, vads):
                if v is not None:
                    v_path = os.path.join(set_path, f"{seq}.vad.npy")
                    with open(v_path, "wb") as numpyfile:
                        np.save(numpyfile, v.astype(np.uint8))
                    vadfile.write(f"{seq} {v_path}\n")
                    frames_in += len(v)
                    frames_out += len(feat)
                    if vad == "drop" and len(feat) == 0:
                        print(f"prepare_numpy_data: {seq} ({path}) has no voiced frame: skipped", file=sys.stderr)
                        skipped += 1
                        continue
                np_path = os.path.join(set_path, f"{seq}.npy")
                with open(np_path, "wb") as numpyfile:
                    np.save(numpyfile, feat)
                featfile.write(f"{seq} {np_path}\n")  # prepare_numpy_data.py:118-119
                lenfile.write(f"{seq} {len(feat)}\n")
                count += 1
                if count % 1000 == 0:
                    print(f"{count} {set_name} files in {time.time() - start_time} seconds.")
            t["write"] += time.time() - t0
    print(f"Processed {count} files in {set_name} set over {time.time() - start_time} seconds.")
    if vad == "drop":
        print("Skipped %d of %d sequences without a voiced frame; dropped %d of %d frames (%.1f%%) in the %s set."
              % (skipped, count + skipped, frames_in - frames_out, frames_in, 100.0 * (frames_in - frames_out) / max(frames_in, 1), set_name))
    if vad is not None:
        return count, (wav_path, feat_path, len_path, vad_path)
    return count, (wav_path, feat_path, len_path)


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("dataset_dir", type=str, help="Directory containing subdirectories with wav.scp files")
    p.add_argument("--np_dir", type=str, default=None, help="Output directory for numpy matrices")
    p.add_argument("--dataset", type=str, default="librispeech", choices=["librispeech", "timit"], help="Dataset name")
    p.add_argument("--set_name", type=str, default=None, help="Set {train, dev, test} to operate on, Leave blank for all three")
    p.add_argument("--ftype", type=str, default="fbank", choices=["fbank", "spec"], help="Feature type to compute")
    p.add_argument("--sr", type=int, default=None,
                   help="Sample rate every file must have (no resampling); default: the rate of the first file")
    p.add_argument("--resample", action="store_true",
                   help="Convert files whose rate differs from --sr (required then) to --sr on the GPU, as librosa.load does")
    p.add_argument("--verify-md5", action="store_true", help="Check every FLAC file's decoded audio against the MD5 it carries")
    p.add_argument("--win_t", type=float, default=0.025, help="Window size in seconds")
    p.add_argument("--hop_t", type=float, default=0.010, help="Frame spacing in seconds")
    p.add_argument("--n_mels", type=int, default=80, help="Number of filter banks if choosing fbank")
    p.add_argument("--vad", type=str, default=None, choices=["mark", "drop"],
                   help="Energy VAD on the GPU: write every sequence's decisions (mark), or also keep the voiced frames only (drop)")
    p.add_argument("--vad_th_ratio", type=float, default=None,
                   help="With --vad: a frame is voiced above this ratio of the mean RMS energy (default 1.04 / 2)")
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.resample and args.sr is None:
        parser.error("--resample needs --sr, the target sample rate")
    if args.vad_th_ratio is not None and args.vad is None:
        parser.error("--vad_th_ratio needs --vad {mark,drop}")
    if args.vad_th_ratio is not None and not (args.vad_th_ratio == args.vad_th_ratio and abs(args.vad_th_ratio) != float("inf")):
        parser.error("--vad_th_ratio must be finite")
    print(args)
    sets = ["train", "dev", "test"] if args.set_name is None else [args.set_name]
    t0 = time.time()
    total = 0
    for s in sets:
        total += prepare_numpy(args.dataset, s, args.dataset_dir, args.np_dir, args.ftype, args.sr, args.win_t, args.hop_t,
                               args.n_mels, resample=args.resample, verify_md5=args.verify_md5, vad=args.vad,
                               vad_th_ratio=features.VAD_TH_RATIO if args.vad_th_ratio is None else args.vad_th_ratio)[0]
    if len(sets) > 1:
        print(f"Processed {total} files in {time.time() - t0} seconds.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
