"""ABX on one MI355X (csrc/abx.hip, pytorch-scalablefhvae_amd/abx.py) -- one JSON line per measurement.

  dtw     fhvae_abx_dtw (max_len = 30: the instance for up to 32 frames; and, as kernel_len64, the one for up to 64) over 10^5, 10^6 and 10^7 pairs (groups of 200 tokens, token lengths uniform on 3 .. 30, frames drawn from
          a pool of 2^18 random rows) at D = 32 and D = 80, angular cost, against the same computation as padded, batched torch
          ops: per chunk of pairs the tokens gathered to (pairs, 64, D), the float64 cosines by bmm, the costs as a
          (pairs, 64, 64) f32 tensor, then an anti-diagonal sweep of 127 steps with the header's tie order.  Both paths
          alternate, --reps runs each, device events around every run: median [min, max] ms and pairs per second.  The torch
          path is run up to --torch-max-pairs (its time grows linearly; above that it is reported as not run).  The largest
          relative difference between the two and the share of bitwise equal pairs are reported.
  scores  abx.evaluate (pair_distances + abx_scores) end to end on a generated token set, host clock: the seconds inside the
          kernel calls and downloads against the seconds of the scoring.

    python tools/bench_abx.py [--reps 10] [--pairs 100000 1000000 10000000] [--dims 32 80] [--torch-max-pairs 1000000]
        [--out profiles/bench_abx.jsonl]
"""
import argparse
import time

import numpy as np

from bench_common import alternate, open_sink, require_gpu, spread  # (importing it sets the package's import path)

GROUP, POOL, LMIN, LMAX, PAD = 200, 1 << 18, 3, 30, 64


def torch_dtw(feats, start, length, ia, ib, chunk=4096):
    """d(token ia[k], token ib[k]) for every k, as batched torch ops (angular cost); the definitions of include/fhvae_abx.h."""
    import torch

    dev = feats.device
    out = torch.empty(ia.shape[0], dtype=torch.float32, device=dev)
    ar = torch.arange(PAD, device=dev)
    inf = torch.tensor(float("inf"), device=dev)
    # cell (i, t - i) of every diagonal t: the column index, clamped, and whether it exists
    tt = torch.arange(2 * PAD - 1, device=dev)[:, None]
    col = (tt - ar[None, :]).clamp(0, PAD - 1)  # (127, 64)
    for c0 in range(0, ia.shape[0], chunk):
        a, b = ia[c0:c0 + chunk], ib[c0:c0 + chunk]
        n, m = length[a].long(), length[b].long()
        ra = (start[a][:, None] + torch.minimum(ar[None, :], n[:, None] - 1))
        rb = (start[b][:, None] + torch.minimum(ar[None, :], m[:, None] - 1))
        A, B = feats[ra].double(), feats[rb].double()  # (P, 64, D), rows past the token repeat its last row
        na, nb = A.square().sum(-1).sqrt(), B.square().sum(-1).sqrt()
        den = na[:, :, None] * nb[:, None, :]
        cos = (torch.bmm(A, B.transpose(1, 2)) / den.clamp_min(1e-300)).clamp(-1.0, 1.0)
        cos = torch.where(den == 0, torch.zeros_like(cos), cos)
        cost = (torch.acos(cos) / np.pi).float()
        del A, B, cos, den
        skew = torch.gather(cost, 2, col.t()[None].expand(cost.shape[0], PAD, 2 * PAD - 1))  # skew[p, i, t] = cost[p, i, t - i]
        P = cost.shape[0]
        d1 = torch.full((P, PAD), float("inf"), device=dev)
        d2, l1, l2 = d1.clone(), torch.zeros(P, PAD, dtype=torch.int32, device=dev), torch.zeros(P, PAD, dtype=torch.int32, device=dev)
        res = torch.zeros(P, device=dev)
        last = n + m - 2
        for t in range(2 * PAD - 1):
            j = t - ar
            live = (j[None, :] >= 0) & (j[None, :] < m[:, None]) & (ar[None, :] < n[:, None])
            up, lup = torch.roll(d1, 1, 1), torch.roll(l1, 1, 1)
            dg, ldg = torch.roll(d2, 1, 1), torch.roll(l2, 1, 1)
            up[:, 0], dg[:, 0] = inf, inf
            left, lleft = torch.where(j[None, :] > 0, d1, inf), l1
            pd, pl = dg, ldg
            pick = up < pd
            pd, pl = torch.where(pick, up, pd), torch.where(pick, lup, pl)
            pick = left < pd
            pd, pl = torch.where(pick, left, pd), torch.where(pick, lleft, pl)
            if t == 0:
                pd, pl = torch.zeros_like(pd), torch.zeros_like(pl)
            d0 = torch.where(live, pd + skew[:, :, t], inf)
            l0 = pl + 1
            end = (last == t)
            if bool(end.any()):
                k = (n - 1)[:, None]
                res = torch.where(end, torch.gather(d0, 1, k)[:, 0] / torch.gather(l0, 1, k)[:, 0].float(), res)
            d2, l2, d1, l1 = d1, l1, d0, l0
        out[c0:c0 + chunk] = res
    return out


def bench_dtw(pairs, D, reps, torch_max, emit):
    import torch

    import abx

    rng = np.random.default_rng(D)
    per = GROUP * (GROUP - 1) // 2
    G = max(1, int(round(pairs / per)))
    N = G * GROUP
    length = rng.integers(LMIN, LMAX + 1, N).astype(np.int32)
    start = rng.integers(0, POOL - LMAX, N).astype(np.int64)
    grp = np.arange(G + 1, dtype=np.int64) * GROUP
    feats = torch.from_numpy(rng.standard_normal((POOL, D)).astype(np.float32)).cuda()
    d_start, d_len = torch.from_numpy(start).cuda(), torch.from_numpy(length).cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.empty(G * GROUP * GROUP, dtype=torch.float32, device="cuda")
    keep = {}

    def kernel():
        keep["k"] = abx.dtw(feats, d_start, d_len, grp, abx.ABX_ANGULAR, status, out=out, max_len=LMAX)

    fns = {"kernel": kernel}
    def kernel64():  # (the instance for tokens of up to 64 frames on the same pairs)
        keep["k64"] = abx.dtw(feats, d_start, d_len, grp, abx.ABX_ANGULAR, status, out=out64)

    out64 = torch.empty_like(out)
    fns["kernel_len64"] = kernel64
    run_torch = G * per <= torch_max
    if run_torch:
        iu = np.triu_indices(GROUP, 1)
        base = (np.arange(G, dtype=np.int64) * GROUP)[:, None]
        ia = torch.from_numpy((base + iu[0][None, :]).reshape(-1)).cuda()
        ib = torch.from_numpy((base + iu[1][None, :]).reshape(-1)).cuda()

        def torch_path():
            keep["t"] = torch_dtw(feats, d_start, d_len, ia, ib)

        fns["torch"] = torch_path
    ts = alternate(fns, reps)
    assert int(status.item()) == 0
    mk = float(np.median(ts["kernel"]))
    cells = float(sum(int(length[g * GROUP:(g + 1) * GROUP].sum()) ** 2 - int((length[g * GROUP:(g + 1) * GROUP].astype(np.int64) ** 2).sum())
                      for g in range(G))) / 2
    res = {"bench": "abx_dtw", "pairs": G * per, "groups": G, "tokens": N, "D": D, "lengths": [LMIN, LMAX], "metric": "angular", "reps": reps,
           "ms_kernel": spread(ts["kernel"]), "ms_kernel_len64": spread(ts["kernel_len64"]),
           "len64_same_bits": bool(torch.equal(keep["k"].view(torch.int32), keep["k64"].view(torch.int32))), "kernel_pairs_per_s": G * per / (mk * 1e-3), "cost_cells": cells,
           "kernel_f64_fma_per_s": cells * D / (mk * 1e-3)}
    if run_torch:
        mt = float(np.median(ts["torch"]))
        got = keep["k"].view(G, GROUP, GROUP)[:, iu[0], iu[1]].reshape(-1)
        rel = ((got.double() - keep["t"].double()).abs() / keep["t"].double()).max()
        res.update(ms_torch=spread(ts["torch"]), torch_pairs_per_s=G * per / (mt * 1e-3), torch_over_kernel=mt / mk,
                   max_rel_diff_vs_torch=float(rel), bitwise_equal_share=float((got.view(torch.int32) == keep["t"].view(torch.int32)).float().mean()))
    else:
        res["torch"] = "not run (above --torch-max-pairs)"
    emit(res)


def bench_scores(reps, emit):
    import torch

    import abx

    rng = np.random.default_rng(1)
    N, P, C, S, D = 20000, 40, 100, 10, 32
    length = rng.integers(LMIN, LMAX + 1, N).astype(np.int32)
    tokens = {"start": rng.integers(0, POOL - LMAX, N).astype(np.int64), "len": length, "phone": rng.integers(0, P, N),
              "ctx": rng.integers(0, C, N), "spk": rng.integers(0, S, N), "phones": ["p%d" % i for i in range(P)],
              "contexts": [("c%d" % i, "x") for i in range(C)], "speakers": ["s%d" % i for i in range(S)], "dropped": {}}
    feats = torch.from_numpy(rng.standard_normal((POOL, D)).astype(np.float32)).cuda()
    t_dist, t_all, res = [], [], None
    for r in range(reps + 1):  # (the first round warms up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        blocks = list(abx.pair_distances(feats, tokens, "angular"))
        t1 = time.perf_counter()
        res = abx.abx_scores(blocks, tokens)
        t2 = time.perf_counter()
        if r:
            t_dist.append(t1 - t0), t_all.append(t2 - t0)
    pairs = int(sum(len(i) * (len(i) - 1) // 2 for _, i, _ in blocks))
    emit({"bench": "abx_evaluate", "tokens": N, "phones": P, "contexts": C, "speakers": S, "D": D, "pairs": pairs, "reps": reps,
          "triples_within": res["triples_within"], "triples_across": res["triples_across"], "cells_within": res["cells_within"],
          "cells_across": res["cells_across"], "s_total": spread(t_all), "s_pair_distances": spread(t_dist),
          "scoring_share": 1.0 - float(np.median(t_dist)) / float(np.median(t_all))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pairs", type=int, nargs="*", default=[100000, 1000000, 10000000])
    ap.add_argument("--dims", type=int, nargs="*", default=[32, 80])
    ap.add_argument("--torch-max-pairs", type=int, default=1000000)
    ap.add_argument("--score-reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch

    require_gpu("bench_abx.py")
    emit = open_sink(args.out)

    for D in args.dims:
        for pairs in args.pairs:
            bench_dtw(pairs, D, args.reps, args.torch_max_pairs, emit)
            torch.cuda.empty_cache()
    if args.score_reps > 0:
        bench_scores(args.score_reps, emit)


if __name__ == "__main__":
    main()
