"""The speaker back end on one MI355X (csrc/spk.hip, spk_backend.py) -- prints one JSON line per measurement.

  pairs    D = 32, 4096 bins, 250 speakers, S = 4 600 / 28 000 / 100 000 rows (tools/bench_sv.py's shapes; centre[spk] + 0.7 randn
           plus one strong nuisance direction).  A back end fitted on at most 20 000 of the rows gives v, a, c.  HIP-event time of
           llr_range, llr_hist (range given) and both, beside hip_binding.sv_hist on the same v rows in the same run (the same
           contraction with a division in its epilogue) and beside the same steps as torch ops in row chunks of at most
           --chunk-elems scores (v[r0:r1] @ v.T + a + a + c, the i < j / label masks, amin / amax and torch.histc per class).
  project  the two stages of Backend.transform at the same S, beside (x - m) @ A.T, the norm, the q sum and the scaling in torch
  trials   llr_trials at 10^5 and 10^6 random pairs of the S = 100 000 rows, beside a torch gather
  fit      spk_backend.fit (host, float64) and score_speakers.py end to end (archives read, fit, all pairs scored, files
           written; host clock) at 100 000 embeddings of 1 000 speakers

Alternated runs, median [min, max] (tools/bench_common.py).

    python tools/bench_spk.py [--reps 10] [--sizes 4600 28000 100000] [--out FILE.jsonl] [--skip-end-to-end]
"""
import argparse
import os
import tempfile
import time

import numpy as np

import bench_common as BC


def make_rows(S, D, speakers, seed):
    rs = np.random.RandomState(seed)
    label = rs.randint(0, speakers, size=S).astype(np.int32)
    n = np.random.RandomState(7).randn(D)
    n /= np.linalg.norm(n)
    x = 3.0 + rs.randn(speakers, D)[label] + 0.7 * rs.randn(S, D) + 4.0 * rs.randn(S, 1) * n
    return x.astype(np.float32), label


def ms(ts, name):
    s = BC.spread(ts[name])
    return {name + "_ms_median": round(s["median"], 3), name + "_ms_min": round(s["min"], 3), name + "_ms_max": round(s["max"], 3)}


def bench_pairs(emit, S, D, NB, speakers, reps, chunk_elems):
    import torch

    import hip_binding as hb
    import spk_backend as SB

    dev = torch.device("cuda")
    x, label = make_rows(S, D, speakers, S)
    sub = slice(0, min(S, 20000))
    t0 = time.perf_counter()
    be = SB.fit(x[sub], label[sub], None, True)
    fit_s = time.perf_counter() - t0
    xd, lab = torch.from_numpy(x).to(dev), torch.from_numpy(label).to(dev)
    v, a = be.transform(xd)
    c = be.c
    r = SB.llr_range(v, a, lab, c).cpu().numpy()
    lo, hi = float(r[:, 0].min()), float(r[:, 1].max())
    status = SB.hip_ext.status_word(dev)
    res = {}
    rows = max(1, min(S, chunk_elems // S))
    col = torch.arange(S, device=dev)

    def torch_pairs():
        hist = torch.zeros((2, NB), dtype=torch.int64, device=dev)
        mn = torch.full((2,), float("inf"), device=dev)
        mx = torch.full((2,), float("-inf"), device=dev)
        for r0 in range(0, S, rows):  # (one pass: the histogram takes the range as given, as the "hist" call does)
            r1 = min(S, r0 + rows)
            sc = (v[r0:r1] @ v.t() + (a[r0:r1, None] + a[None, :])) + c
            upper = col[None, :] > col[r0:r1, None]
            same = lab[r0:r1, None] == lab[None, :]
            for k, sel in ((0, upper & same), (1, upper & ~same)):
                s = sc[sel]
                if s.numel():
                    mn[k], mx[k] = torch.minimum(mn[k], s.min()), torch.maximum(mx[k], s.max())
                    hist[k] += torch.histc(s, bins=NB, min=lo, max=hi).long()
        res["t"] = hist

    fns = {
        "sv_hist": lambda: res.__setitem__("sv", hb.sv_hist(v, lab, NB)),
        "range": lambda: res.__setitem__("r", SB.llr_range(v, a, lab, c, status=status)),
        "hist": lambda: res.__setitem__("h", SB.llr_hist(v, a, lab, c, lo, hi, NB, status=status)),
        "range_hist": lambda: (SB.llr_range(v, a, lab, c, status=status), SB.llr_hist(v, a, lab, c, lo, hi, NB, status=status)),
        "torch": torch_pairs,
    }
    ts = BC.alternate(fns, {"sv_hist": reps, "range": reps, "hist": reps, "range_hist": reps, "torch": max(2, reps // 3)})
    pairs = S * (S - 1) // 2
    k, t = res["h"].cpu().numpy(), res["t"].cpu().numpy()
    assert int(k.sum()) == pairs and int(status.item()) == 0
    # (torch.histc leaves out what its own rounding puts outside [lo, hi]: its totals may fall short by those few trials)
    out = {"what": "spk_pairs", "S": S, "D": D, "bins": NB, "speakers": speakers, "trials": pairs, "reps": reps, "lo": lo, "hi": hi,
           "fit_host_s": round(fit_s, 3), "torch_chunk_rows": rows,
           "largest_cumulative_count_difference": int(np.abs(np.cumsum(k, axis=1) - np.cumsum(t, axis=1)).max()),
           "trials_torch_left_out": int(k.sum() - t.sum())}
    for name in fns:
        out.update(ms(ts, name))
    med = lambda n: float(np.median(ts[n]))  # noqa: E731
    out["hist_over_sv_hist"] = round(med("hist") / med("sv_hist"), 3)
    out["torch_over_range_hist"] = round(med("torch") / med("range_hist"), 2)
    out["hist_gtrials_per_s"] = round(pairs / (med("hist") * 1e-3) / 1e9, 2)
    # the contraction alone: 2 D flop per trial and tile position (the square tiles on the diagonal are computed whole)
    out["hist_tflops_upper_triangle"] = round(2.0 * D * pairs / (med("hist") * 1e-3) / 1e12, 2)
    emit(out)

    # ---- project: both stages
    tab = be._device_tables(dev)
    K1 = int(be.m2.shape[0])

    def torch_project():
        y = (xd - tab["m"]) @ tab["A1"].t()
        y = y * (K1 ** 0.5 / y.norm(dim=1).clamp_min(1e-30))[:, None]
        u = (y - tab["m2"]) @ tab["A_p"].t()
        res["tp"] = (u * tab["sqrt_p"], -(u * u * tab["q"]).sum(dim=1))

    ts = BC.alternate({"project": lambda: res.__setitem__("p", be.transform(xd)), "torch_project": torch_project}, reps)
    err = float((res["p"][0][:, :K1] - res["tp"][0]).abs().max())
    out = {"what": "spk_project", "S": S, "D": D, "K": K1, "reps": reps, "largest_difference_from_torch": err}
    out.update(ms(ts, "project")), out.update(ms(ts, "torch_project"))
    emit(out)
    return v, a, c


def bench_trials(emit, v, a, c, n, reps):
    import torch

    import spk_backend as SB

    S = int(v.shape[0])
    g = torch.Generator(device=v.device).manual_seed(n)
    pairs = torch.randint(0, S, (n, 2), device=v.device, generator=g, dtype=torch.int32)
    res = {}

    def torch_trials():
        i, j = pairs[:, 0].long(), pairs[:, 1].long()
        res["t"] = ((v[i] * v[j]).sum(dim=1) + (a[i] + a[j])) + c

    ts = BC.alternate({"trials": lambda: res.__setitem__("k", SB.llr_trials(v, a, c, pairs)), "torch_trials": torch_trials}, reps)
    out = {"what": "spk_trials", "S": S, "D": int(v.shape[1]), "pairs": n, "reps": reps,
           "largest_difference_from_torch": float((res["k"] - res["t"]).abs().max())}
    out.update(ms(ts, "trials")), out.update(ms(ts, "torch_trials"))
    emit(out)


def bench_end_to_end(emit, S, D, speakers):
    import score_speakers as SS
    import spk_backend as SB

    x, label = make_rows(S, D, speakers, 99)
    t0 = time.perf_counter()
    SB.fit(x, label, None, True)
    fit_s = time.perf_counter() - t0
    with tempfile.TemporaryDirectory() as d:
        for name in ("train", "eval"):
            os.makedirs(os.path.join(d, name))
            np.save(os.path.join(d, name, "mu2.npy"), x)
            with open(os.path.join(d, name, "keys.txt"), "w") as fh:
                fh.writelines("s%04d-%d\n" % (s, n) for n, s in enumerate(label))
        argv = ["--train-emb", os.path.join(d, "train"), "--eval-emb", os.path.join(d, "eval"), "--spk-key-sep", "-", "--backend", "plda",
                "--out", os.path.join(d, "out")]
        t0 = time.perf_counter()
        report = SS.run(SS.parse_args(argv))
        total_s = time.perf_counter() - t0
    emit({"what": "spk_end_to_end", "S": S, "D": D, "speakers": speakers, "fit_host_s": round(fit_s, 3), "score_speakers_s": round(total_s, 3),
          "eer": report["plda"]["eer"], "trials": report["plda"]["n_target"] + report["plda"]["n_nontarget"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4600, 28000, 100000])
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--bins", type=int, default=4096)
    ap.add_argument("--speakers", type=int, default=250)
    ap.add_argument("--chunk-elems", type=int, default=1 << 28, help="scores per row chunk of the torch path (1 GiB of f32)")
    ap.add_argument("--trial-pairs", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--skip-end-to-end", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    BC.require_gpu("bench_spk.py")
    import build_ext

    build_ext.build(verbose=False)
    emit = BC.open_sink(args.out)
    last = None
    for S in args.sizes:
        last = bench_pairs(emit, S, args.dim, args.bins, args.speakers, args.reps, args.chunk_elems)
    for n in args.trial_pairs:
        bench_trials(emit, *last, n, args.reps)
    if not args.skip_end_to_end:
        bench_end_to_end(emit, 100000, args.dim, 1000)


if __name__ == "__main__":
    main()
