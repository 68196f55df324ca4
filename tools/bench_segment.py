"""Times of the segmentation kernels (include/fhvae_segment.h) on one MI355X, against the same computation written as torch ops,
and of discover_units.py with and without --segment.

    python tools/bench_segment.py [--out profiles/bench_segment.jsonl] [--reps 10] [--only kernels|cli]
        [--corpora 1h_10s 10h_10s 1h_one] [--K 50 100 1000] [--D 32 80] [--L 16 32 64] [--torch-dp-steps 20000]

Corpora: 1 h and 10 h of 10 ms frames as 10 s utterances, and 1 h as one utterance; per corpus every K, D and Lmax given.  Per
case, alternated:
  hip_scores   segment.scores (check, norms, room, then per chunk of 4096 rows the sum kernel and the arg-min pass)
  hip_dp       segment.dp on those cells (one wavefront per utterance, the back-trace included)
  hip_segment  segment.segment (both, the grouping, the downloads and the per-utterance arrays on the host)
  torch_scores a float64 cumsum differenced per l, rounded to f32, a matmul and a min, in chunks of 262144 cells (TF32 off)
  torch_dp     the recursion as a loop over t, vectorised over the utterances (equal lengths) and the lengths; without the
               back-trace.  With more than --torch-dp-steps steps (the one-utterance corpus) it is timed over that many steps and
               the line says so: every step costs the same few launches
A line holds the median [min, max] in milliseconds of --reps device-event timings per side after one warm-up, phase 1's share of
the f32 MFMA peak (2 cells K D flop against 157.3 Tflop/s) and phase 2's time per frame step (the median over the longest
utterance's frames: the utterances run side by side), whether torch's units agree and its costs are close.  `cli` writes a corpus to
a temporary directory and times discover_units.py --on feats with and without --segment on a host clock.  One JSON line per case;
no speed is promised.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

from bench_common import ROOT, alternate, open_sink, require_gpu, spread

PEAK_F32_MFMA = 157.3e12
CORPORA = {"1h_10s": (360, 1000), "10h_10s": (3600, 1000), "1h_one": (1, 360000)}


def torch_scores(x, cent, T, L, cells=262144):
    """x (U * T, D) of equal-length utterances -> (score (N, L) f32, unit (N, L) int64): the header's cells with torch ops, in
    chunks of rows that hold about `cells` cells."""
    import torch

    N, D = x.shape
    U, K = N // T, cent.shape[0]
    cs = torch.cumsum(x.view(U, T, D).double(), dim=1)
    cs = torch.cat([cs.new_zeros(U, 1, D), cs], dim=1).view(U * (T + 1), D)  # row u (T + 1) + t: the sum of the rows before t
    cn = (cent * cent).sum(dim=1)
    ls = torch.arange(1, L + 1, device=x.device)
    score = torch.empty(N, L, dtype=torch.float32, device=x.device)
    unit = torch.empty(N, L, dtype=torch.int64, device=x.device)
    per = max(cells // L, 1)
    for a in range(0, N, per):
        n = torch.arange(a, min(a + per, N), device=x.device)
        u, t = n // T, n % T
        first = t[:, None] + 1 - ls[None, :]  # the segment's first row within the utterance
        ok = first >= 0
        base = u * (T + 1)
        S = (cs[base + t + 1][:, None, :] - cs[base[:, None] + first.clamp(min=0)]).float()  # (rows, L, D)
        s = ls[None, :, None].float() * cn[None, None, :] - 2.0 * (S.view(-1, D) @ cent.t()).view(-1, L, K)
        best, k = s.min(dim=2)
        score[a:a + n.shape[0]] = torch.where(ok, best, torch.full_like(best, float("inf")))
        unit[a:a + n.shape[0]] = torch.where(ok, k, torch.full_like(k, -1))
    return score, unit


def torch_dp(score, T, L, lam, steps=None):
    """score (U * T, L) -> (alpha[T] (U,) float64, back (T, U) int8) by a loop over t; `steps`: stop after that many."""
    import torch

    U = score.shape[0] // T
    s3 = score.view(U, T, L).double()
    inf = float("inf")
    hist = torch.full((U, L), inf, dtype=torch.float64, device=score.device)  # column l - 1: alpha[t - l]
    hist[:, 0] = 0.0
    n = T if steps is None else min(T, steps)
    back = torch.empty(n, U, dtype=torch.int8, device=score.device)
    alpha = hist[:, 0]
    for t in range(n):
        v, l = (hist + s3[:, t]).min(dim=1)
        alpha = v + lam
        back[t] = l.to(torch.int8)
        hist = torch.cat([alpha[:, None], hist[:, :-1]], dim=1)
    return alpha, back


def kernel_cases(args, emit):
    import torch

    import segment

    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda:0")
    lam = 1.0
    for name in args.corpora:
        U, T = CORPORA[name]
        for D in args.D:
            g = torch.Generator(device=dev).manual_seed(U + D)
            x = torch.randn(U * T, D, generator=g, device=dev)
            ptr = (torch.arange(U + 1, dtype=torch.int64) * T).to(dev)
            lengths = np.full(U, T, dtype=np.int64)
            for K in args.K:
                cent = torch.randn(K, D, generator=g, device=dev)
                for L in args.L:
                    score, unit = segment.scores(x, cent, ptr, L)
                    steps = T if T <= args.torch_dp_steps else args.torch_dp_steps
                    fns = {"hip_scores": lambda: segment.scores(x, cent, ptr, L),
                           "hip_dp": lambda: segment.dp(score, unit, ptr, lam),
                           "hip_segment": lambda: segment.segment(x, cent, lengths, lam, L),
                           "torch_scores": lambda: torch_scores(x, cent, T, L),
                           "torch_dp": lambda: torch_dp(score, T, L, lam, steps)}
                    ts = alternate(fns, {"hip_scores": args.reps, "hip_dp": args.reps, "hip_segment": args.reps,
                                         "torch_scores": args.torch_reps, "torch_dp": args.torch_reps})
                    tscore, tunit = torch_scores(x, cent, T, L)
                    fin = torch.isfinite(score)
                    agree = float((tunit[fin] == unit[fin].long()).double().mean())
                    worst = float((tscore[fin] - score[fin]).abs().max())
                    line = {"case": "segment_" + name, "utterances": U, "frames": U * T, "K": K, "D": D, "Lmax": L, "lambda": lam,
                            "cells": U * T * L, "torch_units_agree": agree, "torch_scores_max_abs_diff": worst, "torch_dp_steps": steps}
                    if steps == T:
                        cost = segment.dp(score, unit, ptr, lam)[3]
                        line["torch_costs_equal"] = bool((torch_dp(score, T, L, lam)[0].view(torch.int64) == cost.view(torch.int64)).all())
                    for k, v in ts.items():
                        line[k + "_ms"] = spread(v)
                    sec = np.median(ts["hip_scores"]) * 1e-3
                    line["scores_share_of_f32_mfma_peak"] = 2.0 * U * T * L * K * D / sec / PEAK_F32_MFMA
                    line["scores_cells_per_s"] = U * T * L / sec
                    line["dp_us_per_frame_step"] = float(np.median(ts["hip_dp"])) * 1e3 / T
                    line["torch_dp_us_per_frame_step"] = float(np.median(ts["torch_dp"])) * 1e3 / steps
                    emit(line)
                    del score, unit, tscore, tunit
            del x


def cli_case(emit):
    import torch

    import discover_units
    import utils
    from fhvae import FHVAE

    T, F, H, D, U, n = 20, 16, 32, 16, 200, 1000
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "feats.scp"), "w") as fs, open(os.path.join(tmp, "len.scp"), "w") as ls:
            for u in range(U):
                key = "s%02d-%04d" % (u % 10, u)
                np.save(os.path.join(tmp, key + ".npy"), np.repeat(rng.standard_normal((n // 8, F)), 8, axis=0).astype(np.float32)
                        + 0.1 * rng.standard_normal((n, F)).astype(np.float32))
                fs.write("%s %s\n" % (key, os.path.join(tmp, key + ".npy")))
                ls.write("%s %d\n" % (key, n))
        torch.manual_seed(5)
        m = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, num_seqs=U)
        utils.save_checkpoint(m, None, [], {}, "t", 1, 1, 0.0, 0.0, tmp)
        base = ["--checkpoint", os.path.join(tmp, "fhvae_t_e1.tar"), "--feat-scp", os.path.join(tmp, "feats.scp"), "--len-scp",
                os.path.join(tmp, "len.scp"), "--on", "feats", "--k", "50", "--iters", "20"]
        times = {"plain": [], "segment": []}
        for r in range(4):
            for side, extra in (("plain", []), ("segment", ["--segment", "--dur-penalty", "1.0", "--max-seg-frames", "32"])):
                torch.cuda.synchronize()
                t = time.perf_counter()
                code = discover_units.main(base + ["--out", os.path.join(tmp, side)] + extra)
                torch.cuda.synchronize()
                if r:  # (the first round warms up)
                    times[side].append((time.perf_counter() - t) * 1e3)
        info = json.load(open(os.path.join(tmp, "segment", "units.json")))
    emit({"case": "discover_units_cli", "exit": code, "utterances": U, "frames": U * n, "width": F, "k": 50, "iters": 20, "max_seg_frames": 32,
          "plain_wall_ms": spread(times["plain"]), "segment_wall_ms": spread(times["segment"]), "segments": info["segments"]["segments"],
          "mean_frames": info["segments"]["mean_frames"], "bitrate_collapsed": info["bitrate_collapsed"],
          "bitrate_segments": info["segments"]["bitrate_segments"]})


def main(argv=None):
    ap = argparse.ArgumentParser(description="Segmentation kernels against torch ops; discover_units.py with and without --segment")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_segment.jsonl"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=10, help="timings of the torch sides (they are the slow ones)")
    ap.add_argument("--only", default=None, choices=["kernels", "cli"])
    ap.add_argument("--corpora", nargs="+", default=list(CORPORA), choices=list(CORPORA))
    ap.add_argument("--K", nargs="+", type=int, default=[50, 100, 1000])
    ap.add_argument("--D", nargs="+", type=int, default=[32, 80])
    ap.add_argument("--L", nargs="+", type=int, default=[16, 32, 64])
    ap.add_argument("--torch-dp-steps", type=int, default=20000)
    ap.add_argument("--append", action="store_true", help="keep the lines --out holds already")
    args = ap.parse_args(argv)
    require_gpu("bench_segment")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if not args.append:
        open(args.out, "w").close()  # (the sink appends: a run starts the file anew)
    emit = open_sink(args.out)
    if args.only in (None, "kernels"):
        kernel_cases(args, emit)
    if args.only in (None, "cli"):
        cli_case(emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
