"""Exact t-SNE on one MI355X (fhvae_tsne_affinity / fhvae_tsne_step, csrc/tsne.hip) -- prints one JSON line per corpus size.

  D = 32, perplexity 30, 250 clusters, S = 4 600 / 28 000 / 100 000 rows (centre + 0.7 randn).  HIP-event time of the affinity
  launch (hip_binding.tsne_affinity: 50 streaming passes) and of one iteration (hip_binding.tsne_step), alternated in the same
  session with the same steps written as torch ops on the device in row chunks of at most --chunk-elems pairs: for the
  affinities the distances of a chunk and the same 48-step bisection on them (the chunk's distances are kept, which the kernel
  does not do), for the step the distances, both conditional probabilities, the forces and the update.  Median [min, max] over
  --reps alternated runs and the peak device memory of either side above what the inputs take.

    python tools/bench_tsne.py [--reps 10] [--sizes 4600 28000 100000] [--out DIR]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-scalablefhvae_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_sv import event_ms, peak_mb  # noqa: E402


def bench(S, D, perplexity, clusters, reps, chunk_elems):
    import torch

    import hip_binding as hb

    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(S)
    label = torch.randint(0, clusters, (S,), device=dev, generator=g)
    centre = 2.0 * torch.randn((clusters, D), device=dev, generator=g)
    x = centre[label] + 0.7 * torch.randn((S, D), device=dev, generator=g)
    x = (x - x.double().mean(dim=0).float()).contiguous()
    y = 1e-4 * torch.randn((S, 2), device=dev, generator=g)
    lr = max(S / 48.0, 50.0)
    ws = hb.tsne_workspace(x)
    rows = max(1, min(S, chunk_elems // S))
    n = (x * x).sum(dim=1)
    idx = torch.arange(S, device=dev)
    res = {}

    def dist(r0, r1):
        d2 = (n[r0:r1, None] + n[None, :] - 2.0 * (x[r0:r1] @ x.t())).clamp_min_(0.0)
        d2[idx[r0:r1] - r0, idx[r0:r1]] = float("inf")  # j = i takes part in nothing
        return d2

    def k_affinity():
        res["k_aff"] = hb.tsne_affinity(x, perplexity, ws=ws)

    def t_affinity():
        beta, m, z = (torch.empty(S, device=dev) for _ in range(3))
        target = math.log(perplexity)
        for r0 in range(0, S, rows):
            r1 = min(S, r0 + rows)
            d2 = dist(r0, r1)
            mm = d2.min(dim=1).values
            u = d2 - mm[:, None]
            lo, hi = torch.full((r1 - r0,), -60.0, device=dev), torch.full((r1 - r0,), 60.0, device=dev)
            for _ in range(48):
                mid = 0.5 * (lo + hi)
                b = torch.exp2(mid)
                e = torch.exp(-b[:, None] * u)
                s0 = e.sum(dim=1)
                s1 = (e * torch.nan_to_num(u, posinf=0.0)).sum(dim=1)
                up = torch.log(s0) + b * s1 / s0 > target
                lo, hi = torch.where(up, mid, lo), torch.where(up, hi, mid)
            b = torch.exp2(0.5 * (lo + hi))
            beta[r0:r1], m[r0:r1], z[r0:r1] = b, mm, torch.exp(-b[:, None] * u).sum(dim=1)
        res["t_aff"] = (beta, m, z)

    k_affinity(), t_affinity()
    torch.cuda.synchronize()
    beta, m, z = res["k_aff"]
    beta_rel = float(((res["t_aff"][0] - beta).abs() / beta).max())

    def k_step():
        yy, v, gg = y.clone(), torch.zeros_like(y), torch.ones_like(y)
        hb.tsne_step(x, beta, m, z, yy, v, gg, 12.0, 0.5, lr, ws=ws)
        res["k_y"] = yy

    def t_step():
        F, R, W = torch.zeros_like(y), torch.zeros_like(y), torch.zeros(S, device=dev)
        for r0 in range(0, S, rows):
            r1 = min(S, r0 + rows)
            d2 = dist(r0, r1)
            p = (torch.exp(-beta[r0:r1, None] * (d2 - m[r0:r1, None])) / z[r0:r1, None]
                 + torch.exp(-beta[None, :] * (d2 - m[None, :])) / z[None, :]) / (2.0 * S)
            dy0, dy1 = y[r0:r1, 0, None] - y[None, :, 0], y[r0:r1, 1, None] - y[None, :, 1]
            w = 1.0 / (1.0 + dy0 * dy0 + dy1 * dy1)
            w[idx[r0:r1] - r0, idx[r0:r1]] = 0.0
            pw, ww = p * w, w * w
            F[r0:r1, 0], F[r0:r1, 1] = (pw * dy0).sum(dim=1), (pw * dy1).sum(dim=1)
            R[r0:r1, 0], R[r0:r1, 1] = (ww * dy0).sum(dim=1), (ww * dy1).sum(dim=1)
            W[r0:r1] = w.sum(dim=1)
        grad = 4.0 * (12.0 * F - R / W.sum())
        v, gg = torch.zeros_like(y), torch.ones_like(y)
        gg = torch.where(v * grad < 0, gg + 0.2, gg * 0.8).clamp_min(0.01)
        v = 0.5 * v - lr * gg * grad
        res["t_y"] = y + v

    k_step(), t_step()
    torch.cuda.synchronize()
    y_rel = float((res["k_y"] - res["t_y"]).abs().max() / res["t_y"].abs().max())
    mem = {k: peak_mb(f) for k, f in (("kernel_affinity", k_affinity), ("torch_affinity", t_affinity), ("kernel_step", k_step),
                                      ("torch_step", t_step))}
    t = {k: [] for k in mem}
    for _ in range(reps):  # alternated
        for k, f in (("kernel_affinity", k_affinity), ("torch_affinity", t_affinity), ("kernel_step", k_step), ("torch_step", t_step)):
            t[k].append(event_ms(f))
    row = {"what": "tsne", "S": S, "D": D, "perplexity": perplexity, "clusters": clusters, "reps": reps, "torch_chunk_rows": rows,
           "beta_largest_relative_difference": beta_rel, "y_after_one_step_largest_difference_over_max": y_rel}
    for k in t:
        row[k + "_ms_median"], row[k + "_ms_min"], row[k + "_ms_max"] = (round(float(f(t[k])), 3) for f in (np.median, min, max))
        row[k + "_peak_mb"] = round(mem[k], 2)
    row["torch_over_kernel_affinity"] = round(row["torch_affinity_ms_median"] / row["kernel_affinity_ms_median"], 2)
    row["torch_over_kernel_step"] = round(row["torch_step_ms_median"] / row["kernel_step_ms_median"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4600, 28000, 100000])
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--clusters", type=int, default=250)
    ap.add_argument("--chunk-elems", type=int, default=1 << 26, help="pairs per row chunk of the torch path (256 MiB of f32 per array)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to DIR/bench_tsne.jsonl")
    args = ap.parse_args()
    import build_ext

    build_ext.build(verbose=False)
    rows = []
    for S in args.sizes:
        rows.append(bench(S, args.dim, args.perplexity, args.clusters, args.reps, args.chunk_elems))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_tsne.jsonl"), "a") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
