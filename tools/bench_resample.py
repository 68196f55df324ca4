"""Resampling throughput on one MI355X (fhvae_resample_fwd, csrc/resample.hip) -- prints one JSON line per measurement.

  kernel: HIP-event time of one call (check, rows and exception launches) over 10 min and 1 h of seeded audio for
          44.1 -> 16 kHz, 8 -> 16 kHz and 22.05 -> 16 kHz, the time per hour of audio and the share of the 157.3 TFLOP/s
          f32-MFMA peak counting only the necessary 2 * taps FLOP per output sample;
  cli:    wall time of prepare_numpy_data.prepare_numpy over a generated corpus of --corpus-min minutes (default 60) stored
          at 44.1 kHz with resample=True against the same audio stored at 16 kHz without it, alternated --cli-reps times,
          split into read, GPU and write.

    python tools/bench_resample.py [--reps 20] [--corpus-min 60] [--cli-reps 2] [--skip-cli] [--out DIR]
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


def synth(n, sr, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(sr)
    y = np.sin(2 * np.pi * 150 * t) * (0.5 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.05 * rng.standard_normal(n)
    return (0.3 * y).astype(np.float32)


def bench_kernel(sr_in, sr_out, minutes, reps):
    import torch

    import features as F
    import hip_binding as hb

    b = F.resample_bank(sr_in, sr_out)
    utt = 10 * sr_in  # 10 s utterances
    U = max(1, minutes * 6)
    lens = np.full(U, utt, dtype=np.int64)
    olens = F.resampled_length(lens, sr_in, sr_out)
    rows = -(-olens // (b.P * b.L))
    dev = torch.device("cuda")
    ptr = [torch.from_numpy(np.concatenate([[0], np.cumsum(v)]).astype(np.int64)).to(dev) for v in (lens, olens, rows)]
    y = torch.from_numpy(synth(int(lens.sum()), sr_in, minutes)).to(dev)
    bank, chunks = torch.from_numpy(b.bank32).to(dev), torch.from_numpy(b.chunks).to(dev)
    exc = alt = None
    if b.discontinuous:
        exc = torch.from_numpy(b.exceptions(int(-(-olens.max() // b.L))).copy()).to(dev)
        alt = torch.from_numpy(b.alt32).to(dev)
    out = torch.empty(int(olens.sum()), device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def call():
        hb.resample_fwd(y, ptr[0], ptr[1], ptr[2], int(rows.sum()), bank, chunks, b.L, b.M, b.P, b.WL, b.ratio, exc, alt, b.alt_wl,
                        out, status)

    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    assert int(status.item()) == 0
    ms = float(np.median(ts))
    taps = 2 * b.wing
    flop = 2.0 * taps * float(olens.sum())
    done = 2.0 * 16 * float((b.chunks[:, 1] - b.chunks[:, 0]).sum()) * 16 * float(rows.sum())  # FLOP the MFMAs really do
    hours = lens.sum() / sr_in / 3600.0
    return {"what": "resample_kernel", "sr_in": sr_in, "sr_out": sr_out, "audio_min": minutes, "L": b.L, "M": b.M, "P": b.P,
            "KP": b.KP, "taps": taps, "kernel_ms_median": round(ms, 4), "kernel_ms_min": round(float(min(ts)), 4),
            "ms_per_hour_audio": round(ms / hours, 4), "tflops_necessary": round(flop / (ms * 1e-3) / 1e12, 2),
            "frac_f32_mfma_peak": round(flop / (ms * 1e-3) / PEAK_F32_MFMA, 3), "mfma_flop_over_necessary": round(done / flop, 3),
            "reps": reps}


def write_corpus(root, sr, corpus_min):
    d = os.path.join(root, "train")
    os.makedirs(d)
    rng = np.random.default_rng(0)
    total, lines, j = 0.0, [], 0
    while total < corpus_min * 60:
        sec = float(rng.integers(2, 15))  # 2-15 s utterances, the same audio at every rate
        q = np.round(synth(int(sec * sr), sr, j) * 32767).astype("<i2")
        p = os.path.join(d, "u%05d.wav" % j)
        with wave.open(p, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(sr)
            w.writeframes(q.tobytes())
        lines.append("u%05d %s\n" % (j, p))
        total += sec
        j += 1
    with open(os.path.join(d, "wav.scp"), "w") as f:
        f.writelines(lines)
    return total


def bench_cli(corpus_min, root, cli_reps):
    import prepare_numpy_data as P

    rows = []
    secs = {sr: write_corpus(os.path.join(root, "c%d" % sr), sr, corpus_min) for sr in (44100, 16000)}
    for rep in range(cli_reps):
        for sr in (44100, 16000):
            t = {}
            out = os.path.join(root, "np%d_%d" % (sr, rep))
            t0 = time.time()
            count, _ = P.prepare_numpy("bench", "train", os.path.join(root, "c%d" % sr), out, "fbank", 16000, timings=t,
                                       resample=sr != 16000)
            wall = time.time() - t0
            shutil.rmtree(out, ignore_errors=True)
            rows.append({"what": "prepare_numpy_data", "stored_sr": sr, "resample": sr != 16000, "rep": rep,
                         "audio_min": round(secs[sr] / 60, 2), "files": count, "wall_s": round(wall, 3),
                         "read_s": round(t["read"], 3), "gpu_s": round(t["gpu"], 3), "write_s": round(t["write"], 3)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--corpus-min", type=int, default=60)
    ap.add_argument("--cli-reps", type=int, default=2)
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to DIR/bench_resample.jsonl")
    args = ap.parse_args()
    import build_ext

    build_ext.build(verbose=False)
    rows = [bench_kernel(a, 16000, m, args.reps) for a in (44100, 8000, 22050) for m in (10, 60)]
    if not args.skip_cli:
        tmp = tempfile.mkdtemp(prefix="bench_resample_")
        try:
            rows.extend(bench_cli(args.corpus_min, tmp, args.cli_reps))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_resample.jsonl"), "a") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
