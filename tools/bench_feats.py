"""Feature extraction throughput on one MI355X (fhvae_feats_fwd, csrc/feats.hip) -- prints one JSON line per measurement.

  kernel: HIP-event time of one launch over a batch of 1 min, 10 min and 1 h of seeded 16 kHz audio (fbank, 80 mels), the
          time per hour of audio and the TFLOP/s at 2*n_fft*2*n_bins + 2*n_bins*n_mels FLOP per frame against the
          157.3 TFLOP/s f32-MFMA peak;
  cli:    wall time of prepare_numpy_data.prepare_numpy over a generated corpus of --corpus-min minutes (default 60) of
          16-bit WAV files on local disk, split into read, GPU and write.

    python tools/bench_feats.py [--reps 20] [--corpus-min 60] [--skip-cli] [--out DIR]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-scalablefhvae_amd"))

PEAK_F32_MFMA = 157.3e12


def synth(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    y = np.sin(2 * np.pi * 150 * t) * (0.5 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.05 * rng.standard_normal(n)
    return (0.3 * y).astype(np.float32)


def bench_kernel(minutes, reps):
    import torch

    import features as F
    import hip_binding as hb

    sr, n_mels = 16000, 80
    n_fft, hop = F.frame_sizes(sr)
    utt = 10 * sr  # 10 s utterances
    U = max(1, minutes * 60 * sr // utt)
    lens = np.full(U, utt, dtype=np.int64)
    frames = F.num_frames(lens, n_fft, hop)
    dev = torch.device("cuda")
    wave_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).to(dev)
    frame_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(frames)])).to(dev)
    y = torch.from_numpy(synth(int(lens.sum()), minutes)).to(dev)
    dft = torch.from_numpy(F.dft_basis(n_fft)).to(dev)
    mel = torch.from_numpy(F.mel_basis(sr, n_fft, n_mels)).to(dev)
    nf = int(frames.sum())
    out = torch.empty((nf, n_mels), device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    for _ in range(3):
        hb.feats_fwd(y, wave_ptr, frame_ptr, dft, mel, n_fft, hop, n_mels, "fbank", out, status)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hb.feats_fwd(y, wave_ptr, frame_ptr, dft, mel, n_fft, hop, n_mels, "fbank", out, status)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    assert int(status.item()) == 0
    ms = float(np.median(ts))
    n_bins = n_fft // 2 + 1
    flop = nf * (2 * n_fft * 2 * n_bins + 2 * n_bins * n_mels)
    hours = lens.sum() / sr / 3600.0
    return {"what": "feats_kernel", "audio_min": minutes, "frames": nf, "kernel_ms_median": round(ms, 4),
            "kernel_ms_min": round(float(min(ts)), 4), "ms_per_hour_audio": round(ms / hours, 4),
            "tflops": round(flop / (ms * 1e-3) / 1e12, 2), "frac_f32_mfma_peak": round(flop / (ms * 1e-3) / PEAK_F32_MFMA, 3),
            "reps": reps}


def bench_cli(corpus_min, root):
    import prepare_numpy_data as P

    sr = 16000
    d = os.path.join(root, "train")
    os.makedirs(d)
    rng = np.random.default_rng(0)
    total, lines, j = 0, [], 0
    while total < corpus_min * 60 * sr:
        n = int(rng.integers(2 * sr, 15 * sr))  # 2-15 s utterances
        q = np.round(synth(n, j) * 32767).astype("<i2")
        p = os.path.join(d, "u%05d.wav" % j)
        with wave.open(p, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(sr)
            w.writeframes(q.tobytes())
        lines.append("u%05d %s\n" % (j, p))
        total += n
        j += 1
    with open(os.path.join(d, "wav.scp"), "w") as f:
        f.writelines(lines)
    t = {}
    t0 = time.time()
    count, _ = P.prepare_numpy("bench", "train", root, os.path.join(root, "np"), "fbank", sr, timings=t)
    wall = time.time() - t0
    return {"what": "prepare_numpy_data", "audio_min": round(total / sr / 60, 2), "files": count, "wall_s": round(wall, 3),
            "read_s": round(t["read"], 3), "gpu_s": round(t["gpu"], 3), "write_s": round(t["write"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--corpus-min", type=int, default=60)
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to DIR/bench_feats.jsonl")
    args = ap.parse_args()
    import build_ext

    build_ext.build(verbose=False)
    rows = [bench_kernel(m, args.reps) for m in (1, 10, 60)]
    if not args.skip_cli:
        tmp = tempfile.mkdtemp(prefix="bench_feats_")
        try:
            rows.append(bench_cli(args.corpus_min, tmp))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_feats.jsonl"), "a") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
