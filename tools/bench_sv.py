"""All-pairs speaker-verification scoring on one MI355X (fhvae_sv_hist, csrc/sv.hip) -- prints one JSON line per corpus size.

  D = 32, 4096 bins, 250 speakers, S = 4 600 / 28 000 / 100 000 sequences (centre[spk] + 0.7 randn).  HIP-event time of
  hip_binding.sv_hist (workspace and result allocation included), alternated in the same session with the same steps written
  as torch ops on the device: the norms, E[r0:r1] @ E.T in row chunks of at most --chunk-elems scores, the division, the
  i < j / label masks and torch.histc per class and chunk.  Median [min, max] over --reps alternated runs, trials per second
  and the peak device memory of either side above what the inputs take.

    python tools/bench_sv.py [--reps 10] [--sizes 4600 28000 100000] [--out DIR]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-scalablefhvae_amd"))


def event_ms(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def peak_mb(fn):
    """peak device memory of fn() above what is allocated when it starts"""
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def bench(S, D, NB, speakers, reps, chunk_elems):
    import torch

    import hip_binding as hb

    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(S)
    label = torch.randint(0, speakers, (S,), device=dev, generator=g, dtype=torch.int32)
    centre = torch.randn((speakers, D), device=dev, generator=g)
    emb = (centre[label.long()] + 0.7 * torch.randn((S, D), device=dev, generator=g)).contiguous()
    res = {}

    def kernel():
        res["k"] = hb.sv_hist(emb, label, NB)

    rows = max(1, min(S, chunk_elems // S))
    col = torch.arange(S, device=dev)

    def torch_path():
        n = emb.norm(dim=1).clamp_min(1e-30)
        hist = torch.zeros((2, NB), dtype=torch.int64, device=dev)
        for r0 in range(0, S, rows):
            r1 = min(S, r0 + rows)
            sc = (emb[r0:r1] @ emb.t()) / (n[r0:r1, None] * n[None, :])
            upper = col[None, :] > col[r0:r1, None]
            same = label[r0:r1, None] == label[None, :]
            hist[0] += torch.histc(sc[upper & same], bins=NB, min=-1.0, max=1.0).long()
            hist[1] += torch.histc(sc[upper & ~same], bins=NB, min=-1.0, max=1.0).long()
        res["t"] = hist

    kernel(), torch_path()
    torch.cuda.synchronize()
    k, t = res["k"].cpu().numpy(), res["t"].cpu().numpy()
    pairs = S * (S - 1) // 2
    assert int(k.sum()) == pairs and int(t.sum()) == pairs and (k.sum(axis=1) == t.sum(axis=1)).all()
    # trials that histc's own bin arithmetic puts on the other side of an edge: the largest difference of the cumulative counts
    moved = int(np.abs(np.cumsum(k, axis=1) - np.cumsum(t, axis=1)).max())
    k_mb, t_mb = peak_mb(kernel), peak_mb(torch_path)
    tk, tt = [], []
    for _ in range(reps):  # alternated
        tk.append(event_ms(kernel))
        tt.append(event_ms(torch_path))
    k_ms, t_ms = float(np.median(tk)), float(np.median(tt))
    return {"what": "sv_hist", "S": S, "D": D, "bins": NB, "speakers": speakers, "trials": pairs, "reps": reps,
            "kernel_ms_median": round(k_ms, 3), "kernel_ms_min": round(min(tk), 3), "kernel_ms_max": round(max(tk), 3),
            "torch_ms_median": round(t_ms, 3), "torch_ms_min": round(min(tt), 3), "torch_ms_max": round(max(tt), 3),
            "torch_over_kernel": round(t_ms / k_ms, 2), "kernel_gtrials_per_s": round(pairs / (k_ms * 1e-3) / 1e9, 2),
            "torch_gtrials_per_s": round(pairs / (t_ms * 1e-3) / 1e9, 3), "kernel_peak_mb": round(k_mb, 2), "torch_peak_mb": round(t_mb, 1),
            "torch_chunk_rows": rows, "largest_cumulative_count_difference": moved}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4600, 28000, 100000])
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--bins", type=int, default=4096)
    ap.add_argument("--speakers", type=int, default=250)
    ap.add_argument("--chunk-elems", type=int, default=1 << 28, help="scores per row chunk of the torch path (1 GiB of f32)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to DIR/bench_sv.jsonl")
    args = ap.parse_args()
    import build_ext

    build_ext.build(verbose=False)
    rows = []
    for S in args.sizes:
        rows.append(bench(S, args.dim, args.bins, args.speakers, args.reps, args.chunk_elems))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_sv.jsonl"), "a") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
