"""Kaldi fbank throughput on one MI355X (fhvae_kaldi_fbank_fwd, csrc/kaldi_fbank.hip) -- prints one JSON line per measurement.

  kernel: HIP-event time of one launch over a batch of 1 min, 10 min and 1 h of seeded 16 kHz audio (hamming, 80 bins), with
          dither 0 and dither 1, the time per hour of audio and the TFLOP/s at 2*N*2*(P/2) + 2*(P/2)*n_mels FLOP per frame
          against the 157.3 TFLOP/s f32-MFMA peak;
  torch:  the same steps as torch ops (unfold, mean, pre-emphasis, window, torch.fft.rfft, matmul, log) on the same batch,
          timed alternately with the kernel in the same run (dither 0);
  cli:    wall time of prepare_kaldi_data.prepare_kaldi over a generated corpus of --corpus-min minutes (default 60) of
          16-bit WAV files on local disk, split into read, GPU and write.

    python tools/bench_kaldi_fbank.py [--reps 20] [--corpus-min 60] [--skip-cli]
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
OPTS = {"window-type": "hamming", "num-mel-bins": 80, "sample-frequency": 16000}


def synth(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    y = np.sin(2 * np.pi * 150 * t) * (0.5 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.05 * rng.standard_normal(n)
    return np.round(0.3 * 32768 * y).astype(np.float32)  # int16 scale


def torch_fbank(y2d, N, S, P, window, mel_t, c):
    """The torch-op formulation on (U, L) utterances of one length -> (U * frames, n_mels)."""
    import torch

    fr = y2d.unfold(1, N, S)
    fr = fr - fr.mean(dim=2, keepdim=True)
    fr = torch.cat([fr[..., :1] * (1 - c), fr[..., 1:] - c * fr[..., :-1]], dim=2) * window
    spec = torch.fft.rfft(fr, n=P)
    power = (spec.real ** 2 + spec.imag ** 2)[..., :P // 2]
    return torch.log(torch.clamp(power.reshape(-1, P // 2) @ mel_t, min=2.0 ** -23))


def bench_kernel(minutes, reps):
    import torch

    import features as F
    import hip_binding as hb

    o = F.kaldi_fbank_options(OPTS)
    N, S, P = F.kaldi_frame_sizes(o)
    sr, n_mels = 16000, 80
    utt = 10 * sr  # 10 s utterances
    U = max(1, minutes * 60 * sr // utt)
    lens = np.full(U, utt, dtype=np.int64)
    frames = F.kaldi_num_frames(lens, N, S)
    dev = torch.device("cuda")
    wave_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).to(dev)
    frame_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(frames)])).to(dev)
    ids = torch.arange(U, dtype=torch.int64, device=dev)
    y = torch.from_numpy(synth(int(lens.sum()), minutes)).to(dev)
    dft = torch.from_numpy(F.kaldi_dft_basis(N, P, "hamming")).to(dev)
    mel = torch.from_numpy(F.kaldi_mel_basis(sr, P, n_mels)).to(dev)
    window = torch.from_numpy(F.kaldi_window(N, "hamming").astype(np.float32)).to(dev)
    mel_t = torch.from_numpy(F.kaldi_mel_filters(sr, P, n_mels).astype(np.float32).T.copy()).to(dev)
    nf = int(frames.sum())
    out = torch.empty((nf, n_mels), device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def run(dither):
        hb.kaldi_fbank_fwd(y, wave_ptr, frame_ptr, ids, dft, mel, N, S, P, n_mels, 0.97, dither, 1, 7, out, status)

    def run_torch():
        return torch_fbank(y.view(U, utt), N, S, P, window, mel_t, 0.97)

    for _ in range(3):
        run(0.0), run(1.0)
        ref = run_torch()
    torch.cuda.synchronize()
    run(0.0)
    diff = float((out - ref).abs().max())
    ts = {"dither0": [], "dither1": [], "torch": []}
    for _ in range(reps):  # alternated, each timed with its own pair of events
        for name, fn in (("dither0", lambda: run(0.0)), ("torch", run_torch), ("dither1", lambda: run(1.0))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1))
    assert int(status.item()) == 0
    flop = nf * (2.0 * N * 2 * (P // 2) + 2.0 * (P // 2) * n_mels)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    hours = lens.sum() / sr / 3600.0
    return {"bench": "kaldi_fbank_kernel", "audio_min": minutes, "utterances": int(U), "frames": nf, "reps": reps,
            "ms_dither0": med["dither0"], "ms_dither1": med["dither1"], "ms_torch_ops": med["torch"],
            "ms_min_dither0": float(np.min(ts["dither0"])), "ms_max_dither0": float(np.max(ts["dither0"])),
            "ms_per_hour_dither0": med["dither0"] / hours, "ms_per_hour_dither1": med["dither1"] / hours,
            "tflops_dither0": flop / med["dither0"] / 1e9, "peak_fraction_dither0": flop / (med["dither0"] * 1e-3) / PEAK_F32_MFMA,
            "dither_extra_ms": med["dither1"] - med["dither0"], "speedup_over_torch_ops": med["torch"] / med["dither0"],
            "max_abs_diff_vs_torch_ops": diff}


def bench_cli(corpus_min):
    import prepare_kaldi_data as PK

    sr = 16000
    tmp = tempfile.mkdtemp(prefix="kaldi_corpus_")
    try:
        d = os.path.join(tmp, "train")
        os.makedirs(d)
        n_files = corpus_min * 6  # 10 s files
        with open(os.path.join(d, "wav.scp"), "w") as scp:
            for j in range(n_files):
                path = os.path.join(d, "u%05d.wav" % j)
                with wave.open(path, "wb") as w:
                    w.setnchannels(1), w.setsampwidth(2), w.setframerate(sr)
                    w.writeframes(synth(10 * sr, j).astype("<i2").tobytes())
                scp.write("u%05d %s\n" % (j, path))
        conf = os.path.join(tmp, "fbank.conf")
        with open(conf, "w") as fh:
            fh.write("--window-type=hamming\n--num-mel-bins=80\n--dither=1\n")
        PK.prepare_kaldi(tmp, "train", conf)  # warm-up: library load, first launches
        t = {}
        t0 = time.time()
        count, _ = PK.prepare_kaldi(tmp, "train", conf, timings=t)
        wall = time.time() - t0
        return {"bench": "prepare_kaldi_data", "audio_min": corpus_min, "files": count, "wall_s": wall, "read_s": t["read"],
                "gpu_s": t["gpu"], "write_s": t["write"], "x_realtime": corpus_min * 60 / wall}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--corpus-min", type=int, default=60)
    ap.add_argument("--skip-cli", action="store_true")
    args = ap.parse_args()
    for minutes in (1, 10, 60):
        print(json.dumps(bench_kernel(minutes, args.reps)), flush=True)
    if not args.skip_cli:
        print(json.dumps(bench_cli(args.corpus_min)), flush=True)


if __name__ == "__main__":
    main()
