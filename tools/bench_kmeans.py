"""k-means on one MI355X (csrc/kmeans.hip, pytorch-scalablefhvae_amd/units.py) -- one JSON line per measurement.

  assign  fhvae_km_assign (labels only, and with dist) at N = 359 280 (1 h of frames) and 3 592 800 (10 h), K = 50 / 100 / 1000,
          D = 32 / 80, N(0, 1) rows, the centroids K of the rows, against the same step as torch ops: x @ c.T in row chunks of at
          most 1 GiB of scores, * -2 + cn, argmin.  Both paths alternate, --reps runs each, device events around every run:
          median [min, max] ms, the kernel's 2 N K D flop over its time and that as a share of the 157 TFLOP/s f32-MFMA peak (the
          call's time: norm kernels included), and the share of rows both paths label alike.
  update  fhvae_km_update alone (member lists given) and with the stable sort that makes them (units.members), against
          index_add_ of the rows and of ones plus a division, on the labels of the assignment.
  fit     units.fit end to end for 20 iterations (tol below any decrease, so it does not stop early), host clock around a
          device synchronise.

    python tools/bench_kmeans.py [--reps 10] [--rows 359280 3592800] [--cents 50 100 1000] [--dims 32 80] [--fit-reps 3]
        [--out profiles/bench_kmeans.jsonl]
"""
import argparse
import time

import numpy as np

from bench_common import alternate, open_sink, require_gpu, spread  # (importing it sets the package's import path)

PEAK_F32_MFMA = 157e12
SCORE_CHUNK_BYTES = 1 << 30


def torch_assign(x, c):
    import torch

    cn = (c * c).sum(dim=1)
    rows = max(1, SCORE_CHUNK_BYTES // (4 * c.shape[0]))
    out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for r0 in range(0, x.shape[0], rows):
        out[r0:r0 + rows] = (x[r0:r0 + rows] @ c.t()).mul_(-2.0).add_(cn).argmin(dim=1)
    return out


def torch_update(x, labels, K):
    import torch

    sums = torch.zeros(K, x.shape[1], device=x.device).index_add_(0, labels, x)
    count = torch.zeros(K, device=x.device).index_add_(0, labels, torch.ones(labels.shape[0], device=x.device))
    return sums / count.clamp(min=1.0).unsqueeze(1)


def bench_case(N, K, D, reps, emit):
    import torch

    import units

    g = torch.Generator(device="cuda").manual_seed(1000 * D + K)
    x = torch.randn(N, D, device="cuda", generator=g)
    c = x[torch.randperm(N, device="cuda", generator=g)[:K]].contiguous()
    keep = {}

    def labels_only():
        keep["k"] = units.assign(x, c, want_dist=False)[0]

    def with_dist():
        keep["kd"] = units.assign(x, c)

    def torch_path():
        keep["t"] = torch_assign(x, c)

    ts = alternate({"kernel": labels_only, "kernel_dist": with_dist, "torch": torch_path}, reps)
    mk, mt = float(np.median(ts["kernel"])), float(np.median(ts["torch"]))
    flop = 2.0 * N * K * D
    emit({"bench": "km_assign", "N": N, "K": K, "D": D, "reps": reps, "ms_kernel": spread(ts["kernel"]),
          "ms_kernel_with_dist": spread(ts["kernel_dist"]), "ms_torch": spread(ts["torch"]), "torch_over_kernel": mt / mk,
          "kernel_tflops": flop / (mk * 1e-3) / 1e12, "kernel_share_of_f32_mfma_peak": flop / (mk * 1e-3) / PEAK_F32_MFMA,
          "torch_tflops": flop / (mt * 1e-3) / 1e12, "workgroups": (N + 255) // 256,
          "same_labels_share": float((keep["k"].long() == keep["t"]).float().mean())})

    labels, dist = keep["kd"]
    long_labels = labels.long()
    perm, cl_ptr = units.members(labels, K)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    cent = c.clone()

    def kernels():
        keep["u"] = units.update_members(x, perm, cl_ptr, cent, status, dist)

    def with_sort():
        p, q = units.members(labels, K)
        keep["us"] = units.update_members(x, p, q, cent, status, dist)

    def torch_upd():
        keep["tu"] = torch_update(x, long_labels, K)

    ts = alternate({"kernels": kernels, "with_sort": with_sort, "torch": torch_upd}, reps)
    assert int(status.item()) == 0
    mk, ms, mt = (float(np.median(ts[k])) for k in ("kernels", "with_sort", "torch"))
    have = keep["u"][0] > 0
    diff = float((cent[have] - keep["tu"][have]).abs().max())
    emit({"bench": "km_update", "N": N, "K": K, "D": D, "reps": reps, "ms_kernels": spread(ts["kernels"]),
          "ms_with_sort": spread(ts["with_sort"]), "ms_torch_index_add": spread(ts["torch"]), "torch_over_kernels": mt / mk,
          "torch_over_with_sort": mt / ms, "kernels_gb_per_s": N * D * 4 / (mk * 1e-3) / 1e9, "empty_clusters": int((~have).sum()),
          "max_abs_diff_vs_torch": diff})


def bench_fit(N, K, D, reps, emit):
    import torch

    import units

    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(N, D, device="cuda", generator=g)
    secs, res = [], None
    for r in range(reps + 1):  # (the first round warms up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = units.fit(x, K, iters=20, tol=-1.0, seed=0)
        torch.cuda.synchronize()
        if r:
            secs.append(time.perf_counter() - t0)
    emit({"bench": "km_fit", "N": N, "K": K, "D": D, "reps": reps, "iterations": res["iterations"], "s_total": spread(secs),
          "ms_per_iteration": float(np.median(secs)) / res["iterations"] * 1e3, "inertia": res["inertia"], "reseeded": res["reseeded"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, nargs="*", default=[359280, 3592800])
    ap.add_argument("--cents", type=int, nargs="*", default=[50, 100, 1000])
    ap.add_argument("--dims", type=int, nargs="*", default=[32, 80])
    ap.add_argument("--fit-reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch

    require_gpu("bench_kmeans.py")
    emit = open_sink(args.out)

    for D in args.dims:
        for N in args.rows:
            for K in args.cents:
                bench_case(N, K, D, args.reps, emit)
                torch.cuda.empty_cache()
    if args.fit_reps > 0:
        for K in (100, 1000):
            bench_fit(args.rows[0] if args.rows else 359280, K, 32, args.fit_reps, emit)


if __name__ == "__main__":
    main()
