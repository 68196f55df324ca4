"""invert_numpy_data.py -- the inverse of prepare_numpy_data.py: every .npy of a feats.scp -> a WAV file, by Griffin-Lim on
the MI355X (features.synthesize), for --ftype fbank after the mel inversion (features.synthesize_mel).

    python pytorch-scalablefhvae_amd/invert_numpy_data.py FEAT_SCP --out DIR [--sr 16000] [--win_t 0.025] [--hop_t 0.010]
        [--gl_iters 32] [--momentum 0.99] [--gl_seed 0] [--preemphasis 0.97] [--ftype {spec,fbank}] [--n_mels 80]
        [--nnls_iters 200]

FEAT_SCP holds "<seq> <path.npy>" lines.  With --ftype spec (the default) every array must be a (nframes, n_fft // 2 + 1)
log-magnitude spectrogram for the given rate and window ("spec" features; mel "fbank" features cannot be inverted that way).
With --ftype fbank every array must be a (nframes, n_mels) log-mel array: its linear magnitudes are fitted first (non-negative
least squares against the mel bank, --nnls_iters steps).  Writes DIR/<seq>.wav (16-bit PCM mono, hop * (nframes - 1) samples)
in feats.scp order, in chunks of bounded size.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import numpy as np  # noqa: E402

import features  # noqa: E402

CHUNK_FRAMES = features.BATCH_FRAMES  # frames loaded, synthesized and written at a time


def read_scp(path):
    with open(path) as fh:
        return [tuple(line.rstrip().split(None, 1)) for line in fh if line.strip()]


def invert_numpy(feat_scp, out_dir, sr=16000, win_t=0.025, hop_t=0.010, n_iter=32, momentum=0.99, seed=0, preemphasis=0.97,
                 ftype="spec", n_mels=80, nnls_iters=features.NNLS_ITERS):
    """-> the list of WAV paths written."""
    entries = read_scp(feat_scp)
    features.check_synth_params(sr, win_t, hop_t, n_iter, momentum, preemphasis)
    if ftype not in features.FTYPES:
        raise ValueError("ftype must be one of %s, got %r" % (features.FTYPES, ftype))
    if ftype == "fbank":
        features.check_melinv_params(sr, win_t, hop_t, n_mels, nnls_iters)
    os.makedirs(out_dir, exist_ok=True)
    written, t0 = [], time.time()
    chunk, frames = [], 0

    def flush(k):
        names = ["%s (%s)" % e for e in chunk]
        specs = [np.load(path) for _, path in chunk]
        # the chunk number moves the seed on, so that a chunk does not repeat the previous one's phases
        if ftype == "fbank":
            waves = features.synthesize_mel(specs, sr, win_t, hop_t, n_mels=n_mels, nnls_iters=nnls_iters, n_iter=n_iter,
                                            momentum=momentum, preemphasis=preemphasis, seed=seed + k, names=names)
        else:
            waves = features.synthesize(specs, sr, win_t, hop_t, n_iter=n_iter, momentum=momentum, preemphasis=preemphasis,
                                        seed=seed + k, names=names)
        for (seq, _), y in zip(chunk, waves):
            path = os.path.join(out_dir, "%s.wav" % seq)
            features.write_wav(path, y, sr)
            written.append(path)

    k = 0
    for seq, path in entries:
        n = int(np.load(path, mmap_mode="r").shape[0])
        if chunk and frames + n > CHUNK_FRAMES:
            flush(k)
            k += 1
            chunk, frames = [], 0
        chunk.append((seq, path))
        frames += n
    if chunk:
        flush(k)
    print("Synthesized %d files in %.1f seconds." % (len(written), time.time() - t0))
    return written


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("feat_scp", type=str, help="feats.scp written by prepare_numpy_data.py")
    p.add_argument("--out", type=str, required=True, help="Output directory for the WAV files")
    p.add_argument("--sr", type=int, default=16000, help="Sample rate the features were taken at")
    p.add_argument("--win_t", type=float, default=0.025, help="Window size in seconds")
    p.add_argument("--hop_t", type=float, default=0.010, help="Frame spacing in seconds")
    p.add_argument("--gl_iters", type=int, default=32, help="Griffin-Lim rounds")
    p.add_argument("--momentum", type=float, default=0.99, help="Griffin-Lim momentum (0 = the plain algorithm)")
    p.add_argument("--gl_seed", type=int, default=0, help="Seed of the initial phases")
    p.add_argument("--preemphasis", type=float, default=0.97, help="Pre-emphasis to undo (0 = none)")
    p.add_argument("--ftype", type=str, default="spec", choices=list(features.FTYPES)[::-1],
                   help="Feature type of the arrays; fbank: mel inversion in front of Griffin-Lim")
    p.add_argument("--n_mels", type=int, default=80, help="Mel filters of the fbank features")
    p.add_argument("--nnls_iters", type=int, default=features.NNLS_ITERS, help="Steps of the mel inversion (fbank only)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        invert_numpy(args.feat_scp, args.out, args.sr, args.win_t, args.hop_t, args.gl_iters, args.momentum, args.gl_seed,
                     args.preemphasis, args.ftype, args.n_mels, args.nnls_iters)
    except ValueError as e:
        print(str(e), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
