"""The Gaussian mixture on one MI355X (csrc/gmm.hip, pytorch-scalablefhvae_amd/gmm.py) -- one JSON line per measurement.

  passes  fhvae_gmm_loglik, fhvae_gmm_post and fhvae_gmm_stats, each on all N rows in one call, and one whole EM iteration
          (gmm.estep in its default chunks + gmm.mstep) at N = 359 280 (1 h of frames) and 3 592 800 (10 h), K = 50 / 100 / 1000,
          width 32 and 39 (padded to 40), N(0, 1) rows, a model of K of the rows as means, against the same steps as torch ops
          in row chunks of at most 1 GiB of scores: cat(x, x*x) @ tab.T + cst, logsumexp (+ argmax), softmax, post.T @ cat(1, x,
          x*x) summed in float64 over the chunks.  The paths alternate, --reps runs each, device events around every run: median
          [min, max] ms; the passes' 2 N K W flop (W = 2 Dp) and the statistics' 2 N K (W + 1) flop over their time as a share of
          the 157 TFLOP/s f32-MFMA peak; the (N, K) f32 posteriors written (post) or read (stats) over the time as a share of the
          8 TB/s HBM peak; and the largest differences between the two paths' results.
  fit     gmm.fit end to end (k-means start included) on one hour of frames for 10 EM iterations (tol below any fall, so it
          does not stop early), host clock around a device synchronise.

    python tools/bench_gmm.py [--reps 5] [--rows 359280 3592800] [--comps 50 100 1000] [--widths 32 39] [--fit-reps 2]
        [--out profiles/bench_gmm.jsonl]
"""
import argparse
import time

import numpy as np

from bench_common import alternate, open_sink, require_gpu, spread  # (importing it sets the package's import path)

PEAK_F32_MFMA = 157e12
PEAK_HBM = 8e12
SCORE_CHUNK_BYTES = 1 << 30


def chunks(N, K):
    rows = max(1, SCORE_CHUNK_BYTES // (4 * K))
    return [(r0, min(N, r0 + rows)) for r0 in range(0, N, rows)]


def torch_scores(xp, tab, cst, r0, r1):
    import torch

    xc = xp[r0:r1]
    return torch.cat([xc, xc * xc], dim=1) @ tab.t() + cst


def torch_loglik(xp, tab, cst):
    import torch

    N, K = xp.shape[0], tab.shape[0]
    ll = torch.empty(N, dtype=torch.float32, device=xp.device)
    labels = torch.empty(N, dtype=torch.int64, device=xp.device)
    for r0, r1 in chunks(N, K):
        l = torch_scores(xp, tab, cst, r0, r1)
        ll[r0:r1] = torch.logsumexp(l, dim=1)
        labels[r0:r1] = l.argmax(dim=1)
    return ll, labels


def torch_post(xp, tab, cst, out):
    import torch

    for r0, r1 in chunks(xp.shape[0], tab.shape[0]):
        out[r0:r1] = torch.softmax(torch_scores(xp, tab, cst, r0, r1), dim=1)
    return out


def torch_stats(xp, post):
    import torch

    N, K = post.shape
    acc = torch.zeros(K, 1 + 2 * xp.shape[1], dtype=torch.float64, device=xp.device)
    for r0, r1 in chunks(N, K):
        xc = xp[r0:r1]
        acc += (post[r0:r1].t() @ torch.cat([torch.ones(r1 - r0, 1, device=xp.device), xc, xc * xc], dim=1)).double()
    return acc


def torch_em(xp, tab, cst):
    """the three torch steps fused per chunk, as a torch user would write an E-step: no (N, K) matrix is kept"""
    import torch

    N, K = xp.shape[0], tab.shape[0]
    acc = torch.zeros(K, 1 + 2 * xp.shape[1], dtype=torch.float64, device=xp.device)
    total = torch.zeros((), dtype=torch.float64, device=xp.device)
    for r0, r1 in chunks(N, K):
        xc = xp[r0:r1]
        l = torch_scores(xp, tab, cst, r0, r1)
        total += torch.logsumexp(l, dim=1).double().sum()
        acc += (torch.softmax(l, dim=1).t() @ torch.cat([torch.ones(r1 - r0, 1, device=xp.device), xc, xc * xc], dim=1)).double()
    return acc, total


def bench_case(N, K, D, reps, emit):
    import torch

    import gmm

    g = torch.Generator(device="cuda").manual_seed(1000 * D + K)
    x = torch.randn(N, D, device="cuda", generator=g)
    Dp = gmm.padded(D)
    xp = torch.nn.functional.pad(x, (0, Dp - D)).contiguous()
    means = x[torch.randperm(N, device="cuda", generator=g)[:K]].double()
    model = {"weights": torch.full((K,), 1.0 / K, dtype=torch.float64, device="cuda"), "means": means,
             "variances": torch.ones(K, D, dtype=torch.float64, device="cuda")}
    tab, cst = gmm.table(model)
    W = 2 * Dp
    ldp = (K + 3) // 4 * 4
    post = torch.empty(N, ldp, dtype=torch.float32, device="cuda")[:, :K]
    tpost = torch.empty(N, K, dtype=torch.float32, device="cuda")
    gvar = gmm.global_variance(x)
    keep = {}
    keep["ll"] = gmm.loglik(xp, tab, cst)

    def k_loglik():
        keep["ll"] = gmm.loglik(xp, tab, cst)

    def t_loglik():
        keep["tll"] = torch_loglik(xp, tab, cst)

    def k_post():
        gmm.posteriors(xp, tab, cst, keep["ll"][0], out=post)

    def t_post():
        torch_post(xp, tab, cst, tpost)

    def k_stats():
        keep["st"] = gmm.accumulate(xp, post)

    def t_stats():
        keep["tst"] = torch_stats(xp, post)

    def k_em():
        stats, total, _ = gmm.estep(x, model)
        keep["em"] = gmm.mstep(stats, model, N, gvar)

    def t_em():
        keep["tem"] = torch_em(xp, tab, cst)

    ts = alternate({"loglik": k_loglik, "torch_loglik": t_loglik, "post": k_post, "torch_post": t_post, "stats": k_stats,
                    "torch_stats": t_stats, "em_iteration": k_em, "torch_estep": t_em}, reps)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    pass_flop, stats_flop, post_bytes = 2.0 * N * K * W, 2.0 * N * K * (W + 1), 4.0 * N * K
    st, tst = keep["st"], keep["tst"]
    mine = torch.cat([st["nk"][:, None], st["sx"], st["sxx"]], dim=1)
    res = {"bench": "gmm", "N": N, "K": K, "width": D, "Dp": Dp, "reps": reps}
    for name in ts:
        res["ms_" + name] = spread(ts[name])
    res.update({
        "torch_over_kernel": {k: med["torch_" + k] / med[k] for k in ("loglik", "post", "stats")},
        "torch_estep_over_em_iteration": med["torch_estep"] / med["em_iteration"],
        "share_of_f32_mfma_peak": {"loglik": pass_flop / (med["loglik"] * 1e-3) / PEAK_F32_MFMA,
                                   "post": pass_flop / (med["post"] * 1e-3) / PEAK_F32_MFMA,
                                   "stats": stats_flop / (med["stats"] * 1e-3) / PEAK_F32_MFMA},
        "post_traffic_share_of_hbm_peak": {"post": post_bytes / (med["post"] * 1e-3) / PEAK_HBM,
                                           "stats": post_bytes / (med["stats"] * 1e-3) / PEAK_HBM},
        "em_chunks": len(gmm.chunk_rows(N, K, D)),
        "max_abs_diff_loglik_vs_torch": float((keep["ll"][0] - keep["tll"][0]).abs().max()),
        "same_labels_share": float((keep["ll"][1].long() == keep["tll"][1]).float().mean()),
        "max_abs_diff_post_vs_torch": float((post - tpost).abs().max()),
        "max_rel_diff_stats_vs_torch": float(((mine - tst).abs() / (tst.abs() + 1e-3 * N / K)).max())})
    emit(res)


def bench_fit(N, K, D, reps, emit):
    import torch

    import gmm

    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(N, D, device="cuda", generator=g)
    secs, hist = [], None
    for r in range(reps + 1):  # (the first round warms up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, hist = gmm.fit(x, K, iters=10, tol=-1.0, seed=0)
        torch.cuda.synchronize()
        if r:
            secs.append(time.perf_counter() - t0)
    emit({"bench": "gmm_fit", "N": N, "K": K, "width": D, "reps": reps, "iterations": hist["iterations"], "kmeans_iters": 10,
          "s_total": spread(secs), "mean_loglik_first": hist["mean_loglik"][0], "mean_loglik_last": hist["mean_loglik"][-1],
          "starved": hist["starved"], "floored": hist["floored"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="*", default=[359280, 3592800])
    ap.add_argument("--comps", type=int, nargs="*", default=[50, 100, 1000])
    ap.add_argument("--widths", type=int, nargs="*", default=[32, 39])
    ap.add_argument("--fit-reps", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch

    require_gpu("bench_gmm.py")
    emit = open_sink(args.out)

    for D in args.widths:
        for N in args.rows:
            for K in args.comps:
                bench_case(N, K, D, args.reps, emit)
                torch.cuda.empty_cache()
    if args.fit_reps > 0:
        for K in (100, 1000):
            bench_fit(359280, K, 39, args.fit_reps, emit)


if __name__ == "__main__":
    main()
