"""Query-by-example search on one MI355X (csrc/qbe.hip, pytorch-scalablefhvae_amd/qbe.py) -- one JSON line per measurement.

  sdtw    fhvae_qbe_sdtw for 10, 100 and 1000 queries of 20 .. 60 frames against one hour of frames (360 utterances of 1000
          frames of 10 ms) at D = 32 and D = 80, angular cost, without and with the profile outputs (with: the 100 shortest
          queries at most, 2.9 MB of profile each), against the same computation
          as batched torch ops: per query the float64 cosines of all utterances by one matrix product, the costs as a
          (U, n, 1000) f32 tensor, then an anti-diagonal sweep of n + 999 steps, one step per group of ops, with the header's
          tie order.  The paths alternate, --reps runs each, device events around every run: median [min, max] ms.  The torch
          path is run up to --torch-max-queries (its time grows linearly; above that it is reported as not run).  The largest
          relative difference between the two and the share of bitwise equal best costs are reported, and the kernel's float64
          multiply-adds per second as a share of the vector peak (78.6 TFLOP/s: 39.3e12 multiply-adds per second).
  search  qbe.search + qbe.rank_metrics end to end on generated terms, host clock: the seconds inside the kernel calls and
          downloads against the seconds of the scoring.

    python tools/bench_qbe.py [--reps 5] [--queries 10 100 1000] [--dims 32 80] [--torch-max-queries 10] [--torch-reps 2]
        [--out profiles/bench_qbe.jsonl]
"""
import argparse
import time

import numpy as np

from bench_common import alternate, open_sink, require_gpu, spread  # (importing it sets the package's import path)

UTTS, UTT_LEN, QMIN, QMAX, QPOOL = 360, 1000, 20, 60, 1 << 16
F64_PEAK_FMA = 39.3e12  # the float64 vector peak, multiply-adds per second


def torch_sdtw(qfeats, q_start, q_len, feats, U, m):
    """best_cost, best_end (Q, U) as batched torch ops (angular cost): the definitions of include/fhvae_qbe.h, one query against
    all U utterances of m frames at a time."""
    import torch

    dev = feats.device
    Q = len(q_len)
    best, where = torch.empty(Q, U, device=dev), torch.empty(Q, U, dtype=torch.int64, device=dev)
    B = feats.view(U, m, -1).double()
    nb = B.square().sum(-1).sqrt()  # (U, m)
    inf = float("inf")
    for q in range(Q):
        n = int(q_len[q])
        A = qfeats[int(q_start[q]):int(q_start[q]) + n].double()  # (n, D)
        na = A.square().sum(-1).sqrt()
        den = na[None, :, None] * nb[:, None, :]
        cos = (torch.matmul(A[None], B.transpose(1, 2)) / den.clamp_min(1e-300)).clamp(-1.0, 1.0)  # (U, n, m)
        cos = torch.where(den == 0, torch.zeros_like(cos), cos)
        cost = (torch.acos(cos) / np.pi).float()
        del cos, den
        ar = torch.arange(n, device=dev)
        row0 = (ar == 0)[None, :]
        d1 = torch.full((U, n), inf, device=dev)
        d2 = d1.clone()
        l1, l2 = torch.zeros(U, n, dtype=torch.int32, device=dev), torch.zeros(U, n, dtype=torch.int32, device=dev)
        E = torch.empty(U, m, device=dev)
        for t in range(n + m - 1):
            j = t - ar
            live = ((j >= 0) & (j < m))[None, :]
            c = cost[:, ar, j.clamp(0, m - 1)]  # (U, n)
            up, lup = torch.roll(d1, 1, 1), torch.roll(l1, 1, 1)
            pd, pl = torch.roll(d2, 1, 1), torch.roll(l2, 1, 1)
            pick = up < pd
            pd, pl = torch.where(pick, up, pd), torch.where(pick, lup, pl)
            pick = d1 < pd
            pd, pl = torch.where(pick, d1, pd), torch.where(pick, l1, pl)
            pd, pl = torch.where(row0, torch.zeros_like(pd), pd), torch.where(row0, torch.zeros_like(pl), pl)
            d0 = torch.where(live, pd + c, torch.full_like(pd, inf))
            l0 = pl + 1
            if 0 <= t - (n - 1) < m:
                E[:, t - (n - 1)] = d0[:, n - 1] / l0[:, n - 1].float()
            d2, l2, d1, l1 = d1, l1, d0, l0
        best[q], where[q] = E.min(1)
    return best, where


def bench_sdtw(Q, D, reps, torch_max, torch_reps, emit):
    import torch

    import qbe

    rng = np.random.default_rng(1000 * D + Q)
    q_len = rng.integers(QMIN, QMAX + 1, Q).astype(np.int32)
    q_start = rng.integers(0, QPOOL - QMAX, Q).astype(np.int64)
    order = np.argsort(q_len, kind="stable")  # (as qbe.search takes them)
    q_len, q_start = q_len[order], q_start[order]
    qfeats = torch.from_numpy(rng.standard_normal((QPOOL, D)).astype(np.float32)).cuda()
    feats = torch.from_numpy(rng.standard_normal((UTTS * UTT_LEN, D)).astype(np.float32)).cuda()
    utt_ptr = torch.arange(UTTS + 1, dtype=torch.int64, device="cuda") * UTT_LEN
    d_start, d_len = torch.from_numpy(q_start).cuda(), torch.from_numpy(q_len).cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    keep = {}
    out = (torch.empty(Q, UTTS, device="cuda"), torch.empty(Q, UTTS, dtype=torch.int32, device="cuda"),
           torch.empty(Q, UTTS, dtype=torch.int32, device="cuda"), None, None)
    prof_q = min(Q, 100)  # (the profile of 1000 queries is 2.9 GB: measured on the first 100)
    out_p = (torch.empty(prof_q, UTTS, device="cuda"), torch.empty(prof_q, UTTS, dtype=torch.int32, device="cuda"),
             torch.empty(prof_q, UTTS, dtype=torch.int32, device="cuda"), torch.empty(prof_q, UTTS * UTT_LEN, device="cuda"),
             torch.empty(prof_q, UTTS * UTT_LEN, dtype=torch.int32, device="cuda"))

    def kernel():
        keep["k"] = qbe.sdtw(qfeats, d_start, d_len, feats, utt_ptr, qbe.QBE_ANGULAR, status, out=out)

    def kernel_profile():
        keep["p"] = qbe.sdtw(qfeats, d_start[:prof_q], d_len[:prof_q], feats, utt_ptr, qbe.QBE_ANGULAR, status, out=out_p)

    fns, n_reps = {"kernel": kernel, "kernel_profile": kernel_profile}, {"kernel": reps, "kernel_profile": reps}
    run_torch = Q <= torch_max
    if run_torch:
        def torch_path():
            keep["t"] = torch_sdtw(qfeats, q_start, q_len, feats, UTTS, UTT_LEN)

        fns["torch"], n_reps["torch"] = torch_path, torch_reps
    ts = alternate(fns, n_reps)
    assert int(status.item()) == 0
    mk, mp = float(np.median(ts["kernel"])), float(np.median(ts["kernel_profile"]))
    cells = float(q_len.astype(np.int64).sum()) * UTTS * UTT_LEN
    cells_p = float(q_len[:prof_q].astype(np.int64).sum()) * UTTS * UTT_LEN
    fma = cells * D / (mk * 1e-3)
    res = {"bench": "qbe_sdtw", "queries": Q, "utterances": UTTS, "frames": UTTS * UTT_LEN, "D": D, "lengths": [QMIN, QMAX], "metric": "angular",
           "reps": reps, "ms_kernel": spread(ts["kernel"]), "ms_kernel_profile": spread(ts["kernel_profile"]), "profile_queries": prof_q,
           "profile_same_best": bool(all(torch.equal(a.view(torch.int32), b[:prof_q].view(torch.int32)) for a, b in zip(keep["p"][:3], keep["k"][:3]))),
           "cost_cells": cells, "kernel_cells_per_s": cells / (mk * 1e-3), "kernel_profile_cells_per_s": cells_p / (mp * 1e-3),
           "kernel_f64_fma_per_s": fma, "share_of_f64_vector_peak": fma / F64_PEAK_FMA}
    if run_torch:
        mt = float(np.median(ts["torch"]))
        got, (want, where) = keep["k"][0], keep["t"]
        rel = ((got.double() - want.double()).abs() / want.double()).max()
        res.update(torch_reps=torch_reps, ms_torch=spread(ts["torch"]), torch_over_kernel=mt / mk, max_rel_diff_vs_torch=float(rel),
                   bitwise_equal_share=float((got.view(torch.int32) == want.view(torch.int32)).float().mean()),
                   same_end_share=float((keep["k"][2].long() == where).float().mean()))
    else:
        res["torch"] = "not run (above --torch-max-queries)"
    emit(res)


def bench_search(reps, emit):
    import torch

    import qbe

    rng = np.random.default_rng(1)
    Q, D, terms = 100, 32, 20
    feats = torch.from_numpy(rng.standard_normal((UTTS * UTT_LEN, D)).astype(np.float32)).cuda()
    lens = np.full(UTTS, UTT_LEN)
    items = []
    for k in range(Q * 3):  # three tokens per query-to-be: the first max_per_term of every term become queries
        u, at, n = int(rng.integers(0, UTTS)), int(rng.integers(0, UTT_LEN - QMAX)), int(rng.integers(QMIN, QMAX + 1))
        items.append(("u%d" % u, 0.01 * at, 0.01 * (at + n - 1), "t%d" % (k % terms), "-", "-", "s"))
    keys = ["u%d" % u for u in range(UTTS)]
    queries = qbe.queries_from_items(items, keys, lens, max_per_term=Q // terms)
    truth = qbe.truth_from_items(items, keys, lens)
    t_search, t_all, res = [], [], None
    for r in range(reps + 1):  # (the first round warms up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        grid = qbe.search(feats, queries, feats, qbe.utt_ptr_of(lens))
        t1 = time.perf_counter()
        res = qbe.rank_metrics(grid["best_cost"], grid["best_start"], grid["best_end"], queries, truth)
        t2 = time.perf_counter()
        if r:
            t_search.append(t1 - t0), t_all.append(t2 - t0)
    emit({"bench": "qbe_search", "queries": len(queries["id"]), "terms": terms, "utterances": UTTS, "frames": UTTS * UTT_LEN, "D": D, "reps": reps,
          "map": res["map"], "no_target": res["no_target"], "s_total": spread(t_all), "s_search": spread(t_search),
          "scoring_share": 1.0 - float(np.median(t_search)) / float(np.median(t_all))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="*", default=[10, 100, 1000])
    ap.add_argument("--dims", type=int, nargs="*", default=[32, 80])
    ap.add_argument("--torch-max-queries", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--search-reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch

    require_gpu("bench_qbe.py")
    emit = open_sink(args.out)

    for D in args.dims:
        for Q in args.queries:
            bench_sdtw(Q, D, args.reps, args.torch_max_queries, args.torch_reps, emit)
            torch.cuda.empty_cache()
    if args.search_reps > 0:
        bench_search(args.search_reps, emit)


if __name__ == "__main__":
    main()
