"""Times of the CTC forward-backward pass (include/fhvae_ctc.h) on one MI355X, against torch.nn.functional.ctc_loss on the same GPU,
and of one ctc.fit end to end.

    python tools/bench_ctc.py [--out profiles/bench_ctc.jsonl] [--reps 7] [--only loss|fit]

Cases: 1 h and 10 h of 10 ms frames as 10 s utterances of 90 to 110 labels, and 1 h as 60 s utterances of 230 to 250 labels, at
C = 40 and 62 (the blank last); `ctc.loss` without and with the gradient.  The baseline is torch's ctc_loss forward plus backward
through log_softmax on the same logits, in f32 and in float64 (equal-length utterances as one (T, U, C) batch).  If torch's device
path is missing or fails in this build the line says so and the run goes on.

Every time is a host clock around work that ends in a device synchronise, with the inputs already on the device; the sides are
run alternately, `--reps` times each after one warm-up, and a line holds the median [min, max] in milliseconds.  The outputs are
compared: the largest |nll - torch float64| over max(1, |nll|) and the largest gradient difference.  A line also holds the trellis
cells per second and an ESTIMATE of the share of the float64 vector peak (78.6 TFLOP/s, the public figure): per cell the
two sweeps evaluate 7 exponentials and 2 logarithms, counted as 30 float64 operations each, and about 20 additions, comparisons and
selects; per frame and class 2 exponentials and one logarithm per sweep.  One JSON line per case; no speed is promised.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

from bench_common import ROOT  # (importing it sets the package's import path)

sys.path.insert(2, os.path.join(ROOT, "tests"))

PEAK_F64 = 78.6e12
OPS_PER_CELL = 9 * 30 + 20
OPS_PER_FRAME_CLASS = 2 * 3 * 30


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)), "runs": len(ms)}


def timed(fn, sync):
    sync()
    t = time.perf_counter()
    out = fn()
    sync()
    return out, (time.perf_counter() - t) * 1e3


def host_rounds(fns, sync, reps):
    """fns: name -> callable (or None).  -> (name -> times in ms, name -> last output); a side that raises is dropped and named."""
    times, outs, errors = {k: [] for k in fns}, {}, {}
    for k, fn in list(fns.items()):  # the warm-up
        try:
            outs[k], first = timed(fn, sync)
        except Exception as e:  # noqa: BLE001  (a missing device path of the baseline is a result, not a failure of the tool)
            errors[k] = "%s: %s" % (type(e).__name__, str(e)[:200])
            del fns[k]
    for _ in range(reps):
        for k, fn in fns.items():
            outs[k], t = timed(fn, sync)
            times[k].append(t)
    return times, outs, errors


def torch_ctc(z, labels, U, T, L_of, dtype):
    """torch's ctc_loss forward and backward through log_softmax -> (nll (U,), d nll / d z (U T, C))."""
    import torch

    zz = z.to(dtype).reshape(U, T, -1).transpose(0, 1).detach().requires_grad_(True)
    lp = torch.log_softmax(zz, dim=2)
    nll = torch.nn.functional.ctc_loss(lp, labels, torch.full((U,), T, dtype=torch.long), L_of, blank=z.shape[1] - 1, reduction="none")
    nll.sum().backward()
    return nll.detach(), zz.grad.transpose(0, 1).reshape(U * T, -1)


def loss_cases(reps, out):
    import torch

    import ctc
    import hip_ext

    dev = torch.device("cuda:0")
    for C in (40, 62):
        for name, U, T, lo, hi in (("1h_10s", 360, 1000, 90, 110), ("10h_10s", 3600, 1000, 90, 110), ("1h_60s", 60, 6000, 230, 250)):
            rng = np.random.default_rng(C + U)
            lens = rng.integers(lo, hi + 1, U)
            seqs = [rng.integers(0, C - 1, n) for n in lens]
            flat = torch.from_numpy(np.concatenate(seqs).astype(np.int32)).to(dev)
            lab_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
            g = torch.Generator(device=dev).manual_seed(C + U)
            z = 3.0 * torch.randn(U * T, C, generator=g, device=dev)
            ptr = (torch.arange(U + 1, dtype=torch.int64) * T).to(dev)
            padded = torch.zeros(U, hi, dtype=torch.long)
            for u, s in enumerate(seqs):
                padded[u, :len(s)] = torch.from_numpy(s)
            padded, L_of = padded.to(dev), torch.from_numpy(lens).to(torch.long)
            fns = {"hip_nll": lambda: ctc.loss(z, ptr, flat, lab_ptr, C - 1, want_grad=False),
                   "hip_grad": lambda: ctc.loss(z, ptr, flat, lab_ptr, C - 1),
                   "torch_f32": lambda: torch_ctc(z, padded, U, T, L_of, torch.float32),
                   "torch_f64": lambda: torch_ctc(z, padded, U, T, L_of, torch.float64)}
            times, outs, errors = host_rounds(fns, torch.cuda.synchronize, reps)
            cells = int(T * (2 * lens + 1).sum())
            line = {"case": "ctc_" + name, "C": C, "utterances": U, "frames": U * T, "labels": int(lens.sum()), "cells": cells,
                    "ws_groups": len(hip_ext.groups(8 * ctc.cells(ptr.cpu().numpy(), lab_ptr.cpu().numpy()), 1 << 30))}
            for k in ("hip_nll", "hip_grad", "torch_f32", "torch_f64"):
                line[k + "_ms"] = stats(times[k]) if times[k] else None
            line["torch_errors"] = errors
            sec = np.median(times["hip_grad"]) * 1e-3
            line["cells_per_s"] = cells / sec
            line["frames_per_s"] = U * T / sec
            line["f64_peak_share_estimate"] = (cells * OPS_PER_CELL + U * T * C * OPS_PER_FRAME_CLASS) / sec / PEAK_F64
            nll, grad, status = outs["hip_grad"]
            line["status"] = int(status)
            line["nll_bits_equal_without_grad"] = bool((outs["hip_nll"][0].view(torch.int64) == nll.view(torch.int64)).all())
            for k in ("torch_f32", "torch_f64"):
                if k in outs:
                    tn, tg = outs[k]
                    line[k + "_nll_rel_diff"] = float(((tn.double() - nll).abs() / nll.abs().clamp(min=1.0)).max())
                    line[k + "_grad_abs_diff"] = float((tg.double() - grad.double()).abs().max())
            out(line)
            del z, outs


def fit_case(reps, out):
    import torch

    import ctc
    import viterbi_ref

    c = viterbi_ref.corpus(2000, 20, 16, 1.3, 0)
    dev = torch.device("cuda:0")
    x = torch.from_numpy(c["x"]).to(dev)
    ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(c["lengths"])]).astype(np.int64)).to(dev)
    times, outs, _ = host_rounds({"fit": lambda: ctc.fit(x, ptr, c["refs"], 20, iters=100)}, torch.cuda.synchronize, min(reps, 3))
    model, hist = outs["fit"]
    out({"case": "ctc_fit", "utterances": 2000, "frames": int(x.shape[0]), "phones": 20, "width": 16, "fit_ms": stats(times["fit"]),
         "iterations": int(hist["iterations"]), "evaluations": int(hist["evaluations"]), "converged": bool(hist["converged"]),
         "objective": [hist["objective"][0], hist["objective"][-1]],
         "ms_per_evaluation": float(np.median(times["fit"])) / max(1, int(hist["evaluations"]))})


def main(argv=None):
    ap = argparse.ArgumentParser(description="CTC loss and gradient against torch's ctc_loss; one fit end to end")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_ctc.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default=None, choices=["loss", "fit"])
    args = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        print("bench_ctc: needs a MI355X (no CPU fallback)", file=sys.stderr)
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def out(line):
            f.write(json.dumps(line) + "\n")
            f.flush()
            print(json.dumps(line))

        if args.only in (None, "loss"):
            loss_cases(args.reps, out)
        if args.only in (None, "fit"):
            fit_case(args.reps, out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
