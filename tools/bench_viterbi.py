"""Times of the Viterbi decoder and the Levenshtein aligner (include/fhvae_viterbi.h) on one MI355X, against the same recursion as
batched torch ops and against a numpy row-vectorised Levenshtein on the host.

    python tools/bench_viterbi.py [--out profiles/bench_viterbi.jsonl] [--reps 7] [--only vit|edit]

Decoder cases: 1 h and 10 h of 10 ms frames as 10 s utterances, and 1 h as ONE utterance, at C = 40 / 61 / 122.  The baseline is
the header's recursion over the equal-length utterances as torch ops on the same GPU, one `(d[:, :, None] + trans).max(1)` and
one addition per step, then the trace-back by gathers.  Aligner cases: 360 / 3 600 / 36 000 pairs of 20 to 60 reference tokens
whose hypothesis is the reference after random edits; the baseline computes the edit distance only (no counts), row by row.

Every time is a host clock around work that ends in a device synchronise, with the inputs already on the device (the numpy
baseline: on the host); the two sides are run alternately, `--reps` times each after one warm-up (3 times where one baseline run
takes more than 5 s), and a line holds the median [min, max] in milliseconds.  Outputs are compared bitwise in every case: path
and score against the torch recursion (random inputs: no ties, on which torch's max promises no index), S + D + I against the
numpy distance.  One JSON line per case; no speed is promised.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

from bench_common import ROOT  # (importing it sets the package's import path)

FRAMES_PER_UTT = 1000  # 10 s of 10 ms frames


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)), "runs": len(ms)}


def host_pair(ours, base, sync, reps):
    """-> (our times, baseline times, our output, the baseline's output), milliseconds."""
    def timed(fn):
        sync()
        t = time.perf_counter()
        out = fn()
        sync()
        return out, (time.perf_counter() - t) * 1e3

    a, _ = timed(ours)
    b, first = timed(base)
    if first > 5000.0:
        reps = min(reps, 3)
    ta, tb = [], []
    for _ in range(reps):
        a, t = timed(ours)
        ta.append(t)
        b, t = timed(base)
        tb.append(t)
    return ta, tb, a, b


def torch_viterbi(emit, trans, init):
    """emit (U, T, C): the recursion of include/fhvae_viterbi.h as batched torch ops -> (path (U, T) int32, score (U,))."""
    import torch

    U, T, C = emit.shape
    d = init[None, :] + emit[:, 0]
    back = torch.empty(T, U, C, dtype=torch.int64, device=emit.device)
    for t in range(1, T):
        v, back[t] = (d[:, :, None] + trans[None]).max(1)
        d = v + emit[:, t]
    score, q = d.max(1)
    path = torch.empty(U, T, dtype=torch.int64, device=emit.device)
    path[:, T - 1] = q
    for t in range(T - 1, 0, -1):
        q = back[t].gather(1, q[:, None])[:, 0]
        path[:, t - 1] = q
    return path.to(torch.int32), score


def viterbi_cases(reps, out):
    import torch

    import phonerec

    dev = torch.device("cuda:0")
    for C in (40, 61, 122):
        for name, U, T in (("1h_10s", 360, FRAMES_PER_UTT), ("10h_10s", 3600, FRAMES_PER_UTT), ("1h_one", 1, 360 * FRAMES_PER_UTT)):
            g = torch.Generator(device=dev).manual_seed(C + U)
            emit = torch.log_softmax(3.0 * torch.randn(U, T, C, generator=g, device=dev), dim=2)
            trans = torch.log_softmax(torch.randn(C, C, generator=g, device=dev) + 4.0 * torch.eye(C, device=dev), dim=1)
            init = torch.log_softmax(torch.randn(C, generator=g, device=dev), dim=0)
            ptr = (torch.arange(U + 1, dtype=torch.int64) * T).to(dev)
            flat = emit.reshape(U * T, C)
            ta, tb, a, b = host_pair(lambda: phonerec.viterbi(flat, ptr, trans, init), lambda: torch_viterbi(emit, trans, init),
                                     torch.cuda.synchronize, reps)
            same = bool((a[0].reshape(U, T) == b[0]).all()) and bool((a[1].view(torch.int32) == b[1].view(torch.int32)).all())
            line = {"case": "viterbi_" + name, "C": C, "utterances": U, "frames": U * T, "hip_ms": stats(ta), "torch_ms": stats(tb),
                    "bitwise_equal": same, "frames_per_s": U * T / (np.median(ta) * 1e-3)}
            out(line)
            del emit, flat


def numpy_levenshtein(ref, hyp):
    """The edit distance, one vectorised row per reference token (the left-to-right minimum by a running minimum)."""
    m = len(hyp)
    j = np.arange(m + 1)
    row = j.copy()
    for i, r in enumerate(ref, 1):
        cand = np.empty(m + 1, dtype=np.int64)
        cand[0] = i
        cand[1:] = np.minimum(row[:-1] + (hyp != r), row[1:] + 1)
        row = np.minimum.accumulate(cand - j) + j
    return int(row[m])


def edit_pairs(U, seed):
    rng = np.random.default_rng(seed)
    refs, hyps = [], []
    for _ in range(U):
        ref = rng.integers(0, 40, rng.integers(20, 61))
        keep = rng.random(len(ref)) > 0.1
        hyp = np.where(rng.random(len(ref)) < 0.15, rng.integers(0, 40, len(ref)), ref)[keep]
        ins = rng.integers(0, len(hyp) + 1, rng.integers(0, 6))
        refs.append(ref.astype(np.int32))
        hyps.append(np.insert(hyp, ins, rng.integers(0, 40, len(ins))).astype(np.int32))
    return refs, hyps


def edit_cases(reps, out):
    import torch

    import phonerec

    for U in (360, 3600, 36000):
        refs, hyps = edit_pairs(U, U)
        (r, rp), (h, hp) = phonerec.csr(refs, "cuda:0"), phonerec.csr(hyps, "cuda:0")
        ta, tb, a, b = host_pair(lambda: phonerec.align(r, rp, h, hp), lambda: np.array([numpy_levenshtein(x, y) for x, y in zip(refs, hyps)]),
                                 torch.cuda.synchronize, reps)
        counts = a.cpu().numpy().astype(np.int64)
        out({"case": "align", "pairs": U, "ref_tokens": int(sum(len(x) for x in refs)), "hip_ms": stats(ta), "numpy_ms": stats(tb),
             "bitwise_equal": bool(np.array_equal(counts[:, :3].sum(axis=1), b)), "pairs_per_s": U / (np.median(ta) * 1e-3)})


def main(argv=None):
    ap = argparse.ArgumentParser(description="Viterbi decoder and Levenshtein aligner against torch and numpy baselines")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_viterbi.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default=None, choices=["vit", "edit"])
    args = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        print("bench_viterbi: needs a MI355X (no CPU fallback)", file=sys.stderr)
        return 1
    import build_ext

    build_ext.build(verbose=False)
    lines = []

    def out(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    if args.only != "edit":
        viterbi_cases(args.reps, out)
    if args.only != "vit":
        edit_cases(args.reps, out)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    return 0 if all(line["bitwise_equal"] for line in lines) else 2


if __name__ == "__main__":
    sys.exit(main())
