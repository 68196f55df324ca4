"""Mel inversion throughput on one MI355X (fhvae_mel_invert, csrc/melinv.hip) -- prints one JSON line per measurement.

  kernel:     HIP-event time of one launch (200 FISTA steps) over 1 min, 10 min and 1 h of 16 kHz / 80-mel frames, alternated
              in the same session with the same iteration written as torch ops on the device (two matmuls, clamp_min, the
              momentum update, f32), which moves x and y through HBM every step; the ratio of the two; the time per hour of
              audio; and the fraction of the LDS bound the kernel was designed against: per frame and step
              4 n_bins + nnz + n_mels dword reads (2 LDS cycles per wave instruction) and 2 n_bins + n_mels dword writes
              (4 cycles), 256 CUs at 2.4 GHz;
  end to end: wall time of features.synthesize_mel against features.synthesize (32 rounds, transfers both ways) over the same
              frame counts, and the inversion's share of it.

    python tools/bench_melinv.py [--reps 5] [--iters 200] [--rounds 32] [--skip-wall] [--out DIR]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-scalablefhvae_amd"))

CUS, CLOCK = 256, 2.4e9


def event_ms(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def bench_kernel(minutes, reps, iters):
    import torch

    import features as F
    import hip_binding as hb

    sr, n_mels = 16000, 80
    n_fft, hop = F.frame_sizes(sr)
    nf = max(1, minutes * 6) * (10 * sr // hop + 1)  # 10 s utterances
    dev = torch.device("cuda")
    md = F._MelInvDev(sr, n_fft, n_mels, iters, dev)
    A = torch.from_numpy(F.inversion_bank(sr, n_fft, n_mels).astype(np.float32)).to(dev)
    At = A.t().contiguous()
    g = torch.Generator(device=dev).manual_seed(minutes)
    spec = torch.rand((nf, md.n_bins), device=dev, generator=g) ** 4 + 1e-4  # a plausible dynamic range
    mel = (spec @ At).contiguous()
    del spec
    out = torch.empty((nf, md.n_bins), device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    beta = [float(b) for b in md.beta.cpu()]
    inv_l = float(md.inv_l)

    def kernel():
        hb.mel_invert(mel, md.bin_filt, md.bin_w, md.filt_first, md.filt_off, md.filt_w, md.inv_l, md.beta, out, status, in_log=False,
                      out_log=False)

    res = {}

    def torch_loop():
        x = torch.zeros((nf, md.n_bins), device=dev)
        y = torch.zeros_like(x)
        for k in range(iters):
            r = torch.matmul(y, At).sub_(mel)
            xn = torch.addmm(y, r, A, alpha=-inv_l).clamp_min_(0.0)
            y = torch.add(xn, xn - x, alpha=beta[k])
            x = xn
        res["x"] = x

    kernel(), torch_loop()
    torch.cuda.synchronize()
    diff = float((out - res["x"]).abs().max() / res["x"].abs().max())
    tk, tt = [], []
    for _ in range(reps):  # alternated
        tk.append(event_ms(kernel))
        tt.append(event_ms(torch_loop))
    assert int(status.item()) == 0
    k_ms, t_ms = float(np.median(tk)), float(np.median(tt))
    nnz = int(md.filt_w.numel())
    tile = hb.load_library().fhvae_mel_invert_tile_rows(n_mels, md.n_bins)
    cycles = iters * (2 * (4 * md.n_bins + nnz + n_mels) + 4 * (2 * md.n_bins + n_mels))  # LDS cycles per 64 frames
    bound_ms = -(-nf // tile) * cycles * (tile / 64) / CUS / CLOCK * 1e3
    hours = nf * hop / sr / 3600.0
    return {"what": "mel_invert", "audio_min": minutes, "frames": nf, "iters": iters, "kernel_ms_median": round(k_ms, 3),
            "kernel_ms_min": round(min(tk), 3), "torch_loop_ms_median": round(t_ms, 3), "torch_loop_ms_min": round(min(tt), 3),
            "torch_over_kernel": round(t_ms / k_ms, 2), "kernel_s_per_hour_audio": round(k_ms * 1e-3 / hours, 4),
            "lds_bound_ms": round(bound_ms, 3), "frac_lds_bound": round(bound_ms / k_ms, 3),
            "gflops_banded": round(nf * iters * 2 * (2 * nnz + 4 * md.n_bins) / (k_ms * 1e-3) / 1e9, 1),
            "max_rel_diff_to_torch_loop": float("%.3g" % diff), "reps": reps}


def bench_wall(minutes, rounds, iters):
    import torch

    import features as F

    sr = 16000
    n_fft, hop = F.frame_sizes(sr)
    rng = np.random.default_rng(minutes)
    A = F.inversion_bank(sr, n_fft, 80).astype(np.float32)
    mags = [rng.random((10 * sr // hop + 1, n_fft // 2 + 1), dtype=np.float32) ** 4 + 1e-4 for _ in range(max(1, minutes * 6))]
    specs = [np.log(m) for m in mags]
    mels = [np.log(m @ A.T) for m in mags]
    F.synthesize(specs[:1], sr, n_iter=1), F.synthesize_mel(mels[:1], sr, n_iter=1, nnls_iters=iters)
    torch.cuda.synchronize()
    walls = {}
    for name, fn in (("synthesize", lambda: F.synthesize(specs, sr, n_iter=rounds)),
                     ("synthesize_mel", lambda: F.synthesize_mel(mels, sr, n_iter=rounds, nnls_iters=iters)),
                     ("mel_to_spec", lambda: F.mel_to_spec(mels, sr, nnls_iters=iters))):
        t0 = time.time()
        out = fn()
        walls[name] = time.time() - t0
        assert len(out) == len(mels) and all(np.isfinite(o).all() for o in out)
    return {"what": "synthesize_mel", "audio_min": minutes, "rounds": rounds, "iters": iters,
            "synthesize_wall_s": round(walls["synthesize"], 3), "synthesize_mel_wall_s": round(walls["synthesize_mel"], 3),
            "mel_to_spec_wall_s": round(walls["mel_to_spec"], 3),
            "synthesize_mel_wall_s_per_hour_audio": round(walls["synthesize_mel"] * 60.0 / minutes, 3),
            "mel_over_spec": round(walls["synthesize_mel"] / walls["synthesize"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=32)
    ap.add_argument("--skip-wall", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to DIR/bench_melinv.jsonl")
    args = ap.parse_args()
    import build_ext

    build_ext.build(verbose=False)
    rows = []
    for m in (1, 10, 60):
        rows.append(bench_kernel(m, args.reps, args.iters))
        print(json.dumps(rows[-1]), flush=True)
    if not args.skip_wall:
        for m in (1, 10, 60):
            rows.append(bench_wall(m, args.rounds, args.iters))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_melinv.jsonl"), "a") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
