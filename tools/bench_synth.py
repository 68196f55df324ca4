"""Waveform synthesis throughput on one MI355X (fhvae_synth_istft / _project / _deemph, csrc/synth.hip) -- prints one JSON line
per measurement.

  round:      HIP-event times of the two calls of one Griffin-Lim round (inverse STFT, projection with momentum) over a batch
              of 1 min, 10 min and 1 h of 16 kHz frames in 10 s utterances, the time per round per hour of audio and the
              TFLOP/s at 2 * n_fft * 2 * n_bins FLOP per frame and direction against the 157.3 TFLOP/s f32-MFMA peak
              (fhvae_feats_fwd reaches 0.29 of it on the same arithmetic, tools/bench_feats.py);
  synthesize: wall time of features.synthesize (32 rounds, de-emphasis, transfers both ways) over the same batches.

    python tools/bench_synth.py [--reps 10] [--rounds 32] [--skip-wall] [--out DIR]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-scalablefhvae_amd"))

PEAK_F32_MFMA = 157.3e12


def timed(fn, reps):
    import torch

    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts))


def bench_round(minutes, reps):
    import torch

    import features as F
    import hip_binding as hb

    sr = 16000
    n_fft, hop = F.frame_sizes(sr)
    n_bins = n_fft // 2 + 1
    per_utt = 10 * sr // hop + 1  # frames of a 10 s utterance
    U = max(1, minutes * 6)
    frames = np.full(U, per_utt, dtype=np.int64)
    dev = torch.device("cuda")
    wave_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(hop * (frames - 1))])).to(dev)
    frame_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(frames)])).to(dev)
    nf, ns = int(frames.sum()), int(hop * (frames - 1).sum())
    g = torch.Generator(device=dev).manual_seed(minutes)
    mag = torch.rand((nf, n_bins), device=dev, generator=g) + 0.01
    ang = 2 * np.pi * torch.rand((nf, n_bins), device=dev, generator=g)
    cur = torch.stack([mag * torch.cos(ang), mag * torch.sin(ang)], dim=-1).contiguous()
    del ang
    tprev, rebuilt = torch.zeros_like(cur), torch.empty_like(cur)
    ws = torch.empty((nf, (n_fft + 15) // 16 * 16), device=dev)
    y, out = torch.empty(ns, device=dev), torch.empty(ns, device=dev)
    dft = torch.from_numpy(F.dft_basis(n_fft)).to(dev)
    syn = torch.from_numpy(F.synth_basis(n_fft)).to(dev)
    wsq = torch.from_numpy(F.window_sq(n_fft)).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def istft():
        hb.synth_istft(cur, wave_ptr, frame_ptr, syn, wsq, n_fft, hop, ws, y, status)

    def project():
        hb.synth_project(y, wave_ptr, frame_ptr, dft, mag, tprev, 0.99 / 1.99, n_fft, hop, rebuilt, cur, status)

    def deemph():
        hb.synth_deemph(y, wave_ptr, 0.97, out, status)

    for _ in range(2):
        istft(), project(), deemph()
    torch.cuda.synchronize()
    t_i, t_i_min = timed(istft, reps)
    t_p, t_p_min = timed(project, reps)
    t_d, _ = timed(deemph, reps)
    assert int(status.item()) == 0
    flop = nf * 2 * n_fft * 2 * n_bins  # per direction
    hours = ns / sr / 3600.0
    rate = lambda ms: flop / (ms * 1e-3)  # noqa: E731
    return {"what": "synth_round", "audio_min": minutes, "frames": nf, "istft_ms_median": round(t_i, 4), "istft_ms_min": round(t_i_min, 4),
            "project_ms_median": round(t_p, 4), "project_ms_min": round(t_p_min, 4), "deemph_ms_median": round(t_d, 4),
            "round_ms_per_hour_audio": round((t_i + t_p) / hours, 3), "istft_tflops": round(rate(t_i) / 1e12, 2),
            "project_tflops": round(rate(t_p) / 1e12, 2), "istft_frac_f32_mfma_peak": round(rate(t_i) / PEAK_F32_MFMA, 3),
            "project_frac_f32_mfma_peak": round(rate(t_p) / PEAK_F32_MFMA, 3),
            "round_frac_f32_mfma_peak": round(2 * flop / ((t_i + t_p) * 1e-3) / PEAK_F32_MFMA, 3), "reps": reps}


def bench_wall(minutes, rounds):
    import torch

    import features as F

    sr = 16000
    n_fft, hop = F.frame_sizes(sr)
    rng = np.random.default_rng(minutes)
    specs = [np.log(rng.random((10 * sr // hop + 1, n_fft // 2 + 1), dtype=np.float32) + 0.01) for _ in range(max(1, minutes * 6))]
    F.synthesize(specs[:1], sr, n_iter=1)
    torch.cuda.synchronize()
    t0 = time.time()
    out = F.synthesize(specs, sr, n_iter=rounds)
    wall = time.time() - t0
    assert len(out) == len(specs) and all(np.isfinite(o).all() for o in out)
    return {"what": "synthesize", "audio_min": minutes, "rounds": rounds, "wall_s": round(wall, 3),
            "wall_s_per_hour_audio": round(wall * 60.0 / minutes, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=32)
    ap.add_argument("--skip-wall", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to DIR/bench_synth.jsonl")
    args = ap.parse_args()
    import build_ext

    build_ext.build(verbose=False)
    rows = [bench_round(m, args.reps) for m in (1, 10, 60)]
    if not args.skip_wall:
        rows += [bench_wall(m, args.rounds) for m in (1, 10, 60)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_synth.jsonl"), "a") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
