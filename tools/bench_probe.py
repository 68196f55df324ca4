"""The frame probe on one MI355X (csrc/probe.hip, pytorch-scalablefhvae_amd/probe.py) -- one JSON line per measurement.

  passes  fhvae_probe_rows alone, fhvae_probe_grad alone and one probe.objective evaluation (table, both passes, one host sync) at
          N = 359 280 (1 h of frames) and 3 592 800 (10 h), C = 40 / 61 / 1000, width 32 and 80, N(0, 1) rows, N(0, 1 / W) weights,
          uniform labels with a tenth of the rows unlabelled, against the same computation as torch ops in row chunks of at most
          1 GiB of logits: x @ tab.T + cst, log_softmax, nll_loss(sum, ignore_index=-1) (+ argmax) for the forward, and autograd's
          backward onto tab and cst, summed over the chunks, plus the same one host copy for the objective.  The paths alternate,
          --reps runs each, device events around every run: median [min, max] ms; 2 N C W flop per pass (pass 2 executes twice
          that: the logits again and the gradient product) over the time as a share of the 157 TFLOP/s f32-MFMA peak; where torch
          won; and the largest differences between the two paths' results.
  fit     probe.fit end to end on generated blobs (one hour of frames, 40 classes, width 32), host clock around a device synchronise.

    python tools/bench_probe.py [--reps 10] [--rows 359280 3592800] [--classes 40 61 1000] [--widths 32 80] [--fit-reps 2]
        [--out profiles/bench_probe.jsonl]
"""
import argparse
import time

import numpy as np

from bench_common import alternate, open_sink, require_gpu, spread  # (importing it sets the package's import path)

PEAK_F32_MFMA = 157e12
LOGIT_CHUNK_BYTES = 1 << 30


def chunks(N, C):
    rows = max(1, LOGIT_CHUNK_BYTES // (4 * C))
    return [(r0, min(N, r0 + rows)) for r0 in range(0, N, rows)]


def torch_forward(x, y64, tab, cst):
    """-> (sum nll (0-d float64), pred (N,)) without autograd"""
    import torch
    import torch.nn.functional as F

    N, C = x.shape[0], tab.shape[0]
    total = torch.zeros((), dtype=torch.float64, device=x.device)
    pred = torch.empty(N, dtype=torch.int64, device=x.device)
    with torch.no_grad():
        for r0, r1 in chunks(N, C):
            l = x[r0:r1] @ tab.t() + cst
            pred[r0:r1] = l.argmax(dim=1)
            total += F.nll_loss(F.log_softmax(l, dim=1), y64[r0:r1], ignore_index=-1, reduction="sum").double()
    return total, pred


def torch_objective(x, y64, tab, cst, sync):
    """forward and autograd's backward onto tab and cst over the chunks -> (sum nll, grad (C, W + 1)); sync: one host copy"""
    import torch
    import torch.nn.functional as F

    N, C = x.shape[0], tab.shape[0]
    tab = tab.detach().requires_grad_(True)
    cst = cst.detach().requires_grad_(True)
    total = torch.zeros((), dtype=torch.float64, device=x.device)
    for r0, r1 in chunks(N, C):
        loss = F.nll_loss(F.log_softmax(x[r0:r1] @ tab.t() + cst, dim=1), y64[r0:r1], ignore_index=-1, reduction="sum")
        loss.backward()
        total += loss.detach().double()
    grad = torch.cat([tab.grad, cst.grad[:, None]], dim=1)
    if sync:
        return torch.cat([total[None], grad.double().flatten()]).cpu()
    return total, grad


def bench_case(N, C, W, reps, emit):
    import torch

    import probe

    g = torch.Generator(device="cuda").manual_seed(1000 * W + C)
    x = torch.randn(N, W, device="cuda", generator=g)
    tab = (torch.randn(C, W, device="cuda", generator=g) / W ** 0.5).contiguous()
    cst = torch.randn(C, device="cuda", generator=g)
    y = torch.randint(0, C, (N,), device="cuda", generator=g, dtype=torch.int32)
    y[torch.rand(N, device="cuda", generator=g) < 0.1] = -1
    y64 = y.long()
    params = torch.cat([tab, cst[:, None]], dim=1).double().cpu().numpy()
    keep = {"rows": probe.rows(x, y, tab, cst)}

    def k_rows():
        keep["rows"] = probe.rows(x, y, tab, cst)

    def t_forward():
        keep["tfwd"] = torch_forward(x, y64, tab, cst)

    def k_grad():
        keep["grad"] = probe.gradient(x, y, tab, cst, keep["rows"][0])

    def k_objective():
        keep["obj"] = probe.objective(x, y, params, 0.0)

    def t_objective():
        keep["tobj"] = torch_objective(x, y64, tab, cst, True)

    ts = alternate({"rows": k_rows, "torch_forward": t_forward, "gradient": k_grad, "objective": k_objective, "torch_objective": t_objective}, reps)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    flop = 2.0 * N * C * W
    total_t, grad_t = torch_objective(x, y64, tab, cst, False)
    totals = keep["rows"][3].cpu().numpy()
    labelled = float(totals[1])
    res = {"bench": "probe", "N": N, "C": C, "width": W, "reps": reps, "logit_chunks": len(chunks(N, C)),
           "workspace_bytes": probe.ws_bytes(N, C, W), "logits_bytes": 4 * N * C}
    for name in ts:
        res["ms_" + name] = spread(ts[name])
    ratios = {"rows": med["torch_forward"] / med["rows"], "objective": med["torch_objective"] / med["objective"],
              "rows_plus_gradient": med["torch_objective"] / (med["rows"] + med["gradient"])}
    res.update({
        "torch_over_kernel": ratios,
        "torch_won": sorted(k for k, v in ratios.items() if v < 1.0),
        "share_of_f32_mfma_peak": {"rows": flop / (med["rows"] * 1e-3) / PEAK_F32_MFMA,
                                   "gradient_counted": flop / (med["gradient"] * 1e-3) / PEAK_F32_MFMA,
                                   "gradient_executed": 2.0 * flop / (med["gradient"] * 1e-3) / PEAK_F32_MFMA},
        "rel_diff_sum_nll_vs_torch": abs(float(totals[0]) - float(total_t)) / float(total_t),
        "same_pred_share": float((keep["rows"][1].long() == keep["tfwd"][1]).float().mean()),
        "max_abs_diff_mean_grad_vs_torch": float((keep["grad"] - grad_t.double()).abs().max()) / labelled})
    emit(res)


def bench_fit(N, C, D, reps, emit):
    import torch

    import probe

    g = torch.Generator(device="cuda").manual_seed(7)
    centres = torch.randn(C, D, device="cuda", generator=g)
    y = torch.randint(0, C, (N,), device="cuda", generator=g, dtype=torch.int32)
    x = (centres[y.long()] + torch.randn(N, D, device="cuda", generator=g)).contiguous()
    secs, hist, model = [], None, None
    for r in range(reps + 1):  # (the first round warms up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model, hist = probe.fit(x, y, C, iters=100)
        torch.cuda.synchronize()
        if r:
            secs.append(time.perf_counter() - t0)
    emit({"bench": "probe_fit", "N": N, "C": C, "width": D, "reps": reps, "iterations": hist["iterations"], "evaluations": hist["evaluations"],
          "converged": hist["converged"], "s_total": spread(secs), "objective_first": hist["objective"][0],
          "objective_last": hist["objective"][-1], "gradient_norm": hist["gradient_norm"], "train_accuracy": probe.score(x, y, model)["accuracy"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, nargs="*", default=[359280, 3592800])
    ap.add_argument("--classes", type=int, nargs="*", default=[40, 61, 1000])
    ap.add_argument("--widths", type=int, nargs="*", default=[32, 80])
    ap.add_argument("--fit-reps", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch

    require_gpu("bench_probe.py")
    emit = open_sink(args.out)

    for W in args.widths:
        for N in args.rows:
            for C in args.classes:
                bench_case(N, C, W, args.reps, emit)
                torch.cuda.empty_cache()
    if args.fit_reps > 0:
        bench_fit(359280, 40, 32, args.fit_reps, emit)


if __name__ == "__main__":
    main()
