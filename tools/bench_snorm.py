"""Score normalisation on one MI355X (csrc/snorm.hip, csrc/spk.hip's NormScore, score_norm.py) -- prints one JSON line per
measurement.

  cohort   D = 32, S = 4 600 / 28 000 / 100 000 evaluation rows against Nc = 1 000 / 10 000 cohort rows (tools/bench_spk.py's
           rows through a fitted back end), top 200 and 0.  HIP-event time of cohort_stats beside the same figures as torch ops:
           v[r0:r1] @ z.T + a + az + c in row chunks of at most --chunk-elems scores, topk (top > 0), mean and std.
  pairs    norm_range / norm_hist beside spk_backend.llr_range / llr_hist on the same rows in the same run (4096 bins)
  end      score_speakers.py --snorm end to end (archives read, fit, cohort made, all pairs scored twice, files written; host
           clock) at 100 000 embeddings of 1 000 speakers, beside the same run without --snorm

Alternated runs, median [min, max] (tools/bench_common.py).

    python tools/bench_snorm.py [--reps 10] [--sizes 4600 28000 100000] [--cohorts 1000 10000] [--tops 200 0] [--out FILE.jsonl]
        [--skip-end-to-end]
"""
import argparse
import os
import tempfile
import time

import numpy as np

import bench_common as BC
from bench_spk import make_rows, ms


def bench_cohort(emit, be, v, a, lab, S, Nc, top, D, speakers, reps, chunk_elems):
    import torch

    import score_norm as SN

    dev = v.device
    xc, _ = make_rows(Nc, D, speakers, 7000 + Nc)
    z, az = be.transform(torch.from_numpy(xc).to(dev))
    c = float(np.float32(be.c))
    K = Nc if top <= 0 else min(top, Nc)
    status = SN.hip_ext.status_word(dev)
    rows = max(1, min(S, chunk_elems // Nc))
    res = {}

    def torch_stats():
        mu, sd, thr = (torch.empty(S, device=dev) for _ in range(3))
        for r0 in range(0, S, rows):
            r1 = min(S, r0 + rows)
            sc = (v[r0:r1] @ z.t() + (a[r0:r1, None] + az[None, :])) + c
            if K < Nc:
                sc = torch.topk(sc, K, dim=1).values
                thr[r0:r1] = sc[:, K - 1]
            else:
                thr[r0:r1] = sc.amin(dim=1)
            mu[r0:r1], sd[r0:r1] = sc.mean(dim=1), sc.std(dim=1, unbiased=False)
        res["t"] = (mu, sd, thr)

    fns = {"cohort_stats": lambda: res.__setitem__("k", SN.cohort_stats(v, a, z, az, c, top, status=status)), "torch": torch_stats}
    ts = BC.alternate(fns, {"cohort_stats": reps, "torch": max(2, reps // 2)})
    assert int(status.item()) == 0
    mu, sd, _, thr = res["k"]
    out = {"what": "sn_cohort", "S": S, "Nc": Nc, "top": top, "K": K, "D": D, "reps": reps, "torch_chunk_rows": rows,
           "largest_difference_from_torch": {"mu": float((mu - res["t"][0]).abs().max()), "sd": float((sd - res["t"][1]).abs().max()),
                                             "thr": float((thr - res["t"][2]).abs().max())}}
    out.update(ms(ts, "cohort_stats")), out.update(ms(ts, "torch"))
    med = lambda n: float(np.median(ts[n]))  # noqa: E731
    out["torch_over_cohort_stats"] = round(med("torch") / med("cohort_stats"), 3)
    out["gscores_per_s"] = round(S * Nc / (med("cohort_stats") * 1e-3) / 1e9, 2)  # (every score is computed seven times)
    emit(out)
    return res["k"]


def bench_pairs(emit, be, v, a, lab, mu, r, S, D, NB, reps):
    import score_norm as SN
    import spk_backend as SB

    c = float(np.float32(be.c))
    status = SN.hip_ext.status_word(v.device)
    rr = SB.llr_range(v, a, lab, c).cpu().numpy()
    lo, hi = float(rr[:, 0].min()), float(rr[:, 1].max())
    rn = SN.norm_range(v, a, mu, r, lab, c).cpu().numpy()
    nlo, nhi = float(rn[:, 0].min()), float(rn[:, 1].max())
    res = {}
    fns = {
        "llr_range": lambda: SB.llr_range(v, a, lab, c, status=status),
        "sn_range": lambda: SN.norm_range(v, a, mu, r, lab, c, status=status),
        "llr_hist": lambda: res.__setitem__("h", SB.llr_hist(v, a, lab, c, lo, hi, NB, status=status)),
        "sn_hist": lambda: res.__setitem__("n", SN.norm_hist(v, a, mu, r, lab, c, nlo, nhi, NB, status=status)),
    }
    ts = BC.alternate(fns, reps)
    pairs = S * (S - 1) // 2
    assert int(res["h"].sum()) == pairs == int(res["n"].sum()) and int(status.item()) == 0
    out = {"what": "sn_pairs", "S": S, "D": D, "bins": NB, "trials": pairs, "reps": reps}
    for name in fns:
        out.update(ms(ts, name))
    med = lambda n: float(np.median(ts[n]))  # noqa: E731
    out["sn_hist_over_llr_hist"] = round(med("sn_hist") / med("llr_hist"), 3)
    out["sn_range_over_llr_range"] = round(med("sn_range") / med("llr_range"), 3)
    emit(out)


def bench_end_to_end(emit, S, D, speakers, top):
    import score_speakers as SS

    x, label = make_rows(S, D, speakers, 99)
    with tempfile.TemporaryDirectory() as d:
        for name in ("train", "eval"):
            os.makedirs(os.path.join(d, name))
            np.save(os.path.join(d, name, "mu2.npy"), x)
            with open(os.path.join(d, name, "keys.txt"), "w") as fh:
                fh.writelines("s%04d-%d\n" % (s, n) for n, s in enumerate(label))
        argv = ["--train-emb", os.path.join(d, "train"), "--eval-emb", os.path.join(d, "eval"), "--spk-key-sep", "-", "--backend", "plda"]
        took = {}
        for name, extra in (("plain", []), ("snorm", ["--snorm", "--snorm-top", str(top)])):
            t0 = time.perf_counter()
            report = SS.run(SS.parse_args(argv + ["--out", os.path.join(d, name)] + extra))
            took[name] = time.perf_counter() - t0
    sn = report["plda"]["snorm"]
    emit({"what": "sn_end_to_end", "S": S, "D": D, "speakers": speakers, "top": sn["top"], "cohort": sn["cohort"],
          "score_speakers_s": round(took["plain"], 3), "score_speakers_snorm_s": round(took["snorm"], 3), "eer": report["plda"]["eer"],
          "eer_snorm": sn["eer"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4600, 28000, 100000])
    ap.add_argument("--cohorts", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--tops", type=int, nargs="+", default=[200, 0])
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--bins", type=int, default=4096)
    ap.add_argument("--speakers", type=int, default=250)
    ap.add_argument("--chunk-elems", type=int, default=1 << 28, help="scores per row chunk of the torch path (1 GiB of f32)")
    ap.add_argument("--skip-end-to-end", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    BC.require_gpu("bench_snorm.py")
    import build_ext

    build_ext.build(verbose=False)
    import torch

    import spk_backend as SB

    emit = BC.open_sink(args.out)
    dev = torch.device("cuda")
    for S in args.sizes:
        x, label = make_rows(S, args.dim, args.speakers, S)
        sub = slice(0, min(S, 20000))
        be = SB.fit(x[sub], label[sub], None, True)
        v, a = be.transform(torch.from_numpy(x).to(dev))
        lab = torch.from_numpy(label).to(dev)
        stats = None
        for Nc in args.cohorts:
            for top in args.tops:
                stats = bench_cohort(emit, be, v, a, lab, S, Nc, top, args.dim, args.speakers, args.reps, args.chunk_elems)
        bench_pairs(emit, be, v, a, lab, stats[0], stats[2], S, args.dim, args.bins, args.reps)
    if not args.skip_end_to_end:
        bench_end_to_end(emit, 100000, args.dim, 1000, 200)


if __name__ == "__main__":
    main()
