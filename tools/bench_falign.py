"""Times of the forced-alignment pass (include/fhvae_falign.h) on one MI355X, against the nll-only CTC pass on the same batch and
against the same computation written as batched torch ops, and of align_phones.py end to end.

    python tools/bench_falign.py [--out profiles/bench_falign.jsonl] [--reps 10] [--only align|cli]

Cases (tools/bench_ctc.py's shapes): 1 h and 10 h of 10 ms frames as 10 s utterances of 90 to 110 labels, and 1 h as 60 s
utterances of 230 to 250 labels, at C = 40 and 62, in CTC topology (the blank last) and in HMM topology.  Per case, alternated:
  hip_align    falign.align (the check kernel, the four sweeps with their trace-back, one status read)
  hip_ctc_nll  ctc.loss(..., want_grad=False) on the same batch (CTC topology only): the sum-product twin of the sweep
  torch        a padded (U, S) max-plus sweep with a gather per frame, int8 back-pointers and a trace-back, all utterances at once
  torchaudio   torchaudio.functional.forced_align, only if `import torchaudio` succeeds; otherwise the line says it is not installed
A line holds the median [min, max] in milliseconds of --reps device-event timings per side after one warm-up, the trellis cells
per second, and whether torch's states and scores equal the kernel's.  `cli` writes the generator's corpus to a temporary
directory and times align_phones.py (fit + alignment + files) on a host clock.  One JSON line per case; no speed is promised.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

from bench_common import ROOT, alternate, open_sink, require_gpu, spread

sys.path.insert(2, os.path.join(ROOT, "tests"))


def torch_align(z3, ext, skip, n_states, n_start, ctc_topology):
    """z3 (U, T, C) f32, ext (U, S) int64 padded with class 0, skip (U, S) bool, n_states (U,) -> (state (U, T) int64, score (U,)).
    The header's recursion over all utterances at once: float64, the smallest k of the largest candidate."""
    import torch

    U, T, _ = z3.shape
    S = ext.shape[1]
    dev = z3.device
    neg = torch.full((U, 2), -float("inf"), dtype=torch.float64, device=dev)
    valid = torch.arange(S, device=dev)[None, :] < n_states[:, None]
    pen = torch.where(skip, 0.0, -float("inf")).to(torch.float64)
    delta = torch.where(valid & (torch.arange(S, device=dev)[None, :] < n_start), z3[:, 0].gather(1, ext).double(), neg[:, :1])
    back = torch.zeros(T, U, S, dtype=torch.int8, device=dev)
    for t in range(1, T):
        p = torch.cat([neg, delta], dim=1)
        cand = torch.stack([delta, p[:, 1:S + 1], p[:, :S] + pen])
        best, k = cand.max(dim=0)  # (the first index of equal maxima on this build; the outputs are compared below)
        back[t] = k.to(torch.int8)
        delta = torch.where(valid, best + z3[:, t].gather(1, ext).double(), neg[:, :1])
    last = (n_states - 1).clamp(min=0)
    v1 = delta.gather(1, last[:, None])[:, 0]
    q = last
    score = v1
    if ctc_topology:
        prev = (n_states - 2).clamp(min=0)
        v2 = torch.where(n_states >= 2, delta.gather(1, prev[:, None])[:, 0], neg[:, 0])
        q = torch.where(v2 > v1, prev, last)
        score = torch.maximum(v1, v2)
    state = torch.empty(U, T, dtype=torch.int64, device=dev)
    for t in range(T - 1, -1, -1):
        state[:, t] = q
        q = (q - back[t].gather(1, q[:, None])[:, 0].long()).clamp(min=0)
    return state, score


def align_cases(reps, emit):
    import torch

    import ctc
    import falign

    try:
        import torchaudio  # noqa: F401
        have_ta = True
    except Exception:  # noqa: BLE001
        have_ta = False
    dev = torch.device("cuda:0")
    for C in (40, 62):
        for name, U, T, lo, hi in (("1h_10s", 360, 1000, 90, 110), ("10h_10s", 3600, 1000, 90, 110), ("1h_60s", 60, 6000, 230, 250)):
            for topology in ("ctc", "hmm"):
                rng = np.random.default_rng(C + U)
                lens = rng.integers(lo, hi + 1, U)
                seqs = [rng.integers(0, C - 1, n) for n in lens]
                blank = C - 1 if topology == "ctc" else -1
                flat = torch.from_numpy(np.concatenate(seqs).astype(np.int32)).to(dev)
                lab_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
                g = torch.Generator(device=dev).manual_seed(C + U)
                z = 3.0 * torch.randn(U * T, C, generator=g, device=dev)
                ptr = (torch.arange(U + 1, dtype=torch.int64) * T).to(dev)
                n_states = torch.from_numpy(2 * lens + 1 if topology == "ctc" else lens).to(dev)
                S = int(n_states.max())
                ext, skip = np.zeros((U, S), dtype=np.int64), np.zeros((U, S), dtype=bool)
                for u, s in enumerate(seqs):
                    if topology == "ctc":
                        ext[u, :2 * len(s) + 1] = blank
                        ext[u, 1:2 * len(s):2] = s
                        skip[u, 3:2 * len(s):2] = s[1:] != s[:-1]
                    else:
                        ext[u, :len(s)] = s
                ext, skip = torch.from_numpy(ext).to(dev), torch.from_numpy(skip).to(dev)
                z3 = z.view(U, T, C)
                fns = {"hip_align": lambda: falign.align(z, ptr, flat, lab_ptr, blank),
                       "torch": lambda: torch_align(z3, ext, skip, n_states, 2 if topology == "ctc" else 1, topology == "ctc")}
                if topology == "ctc":
                    fns["hip_ctc_nll"] = lambda: ctc.loss(z, ptr, flat, lab_ptr, blank, want_grad=False)
                if have_ta and topology == "ctc":
                    import torchaudio

                    lp = torch.log_softmax(z3, dim=2)
                    fns["torchaudio"] = lambda: [torchaudio.functional.forced_align(lp[u:u + 1], torch.from_numpy(seqs[u])[None].to(dev), blank=blank)
                                                 for u in range(U)]
                ts = alternate(fns, reps)
                state, seg, score, bits = falign.align(z, ptr, flat, lab_ptr, blank)
                tstate, tscore = torch_align(z3, ext, skip, n_states, 2 if topology == "ctc" else 1, topology == "ctc")
                cells = int(T * n_states.sum())
                sec = np.median(ts["hip_align"]) * 1e-3
                line = {"case": "falign_" + name, "topology": topology, "C": C, "utterances": U, "frames": U * T, "labels": int(lens.sum()),
                        "cells": cells, "status": int(bits), "cells_per_s": cells / sec, "frames_per_s": U * T / sec,
                        "torchaudio": "measured" if "torchaudio" in fns else ("not installed" if not have_ta else "CTC topology only"),
                        "torch_states_equal": bool((tstate.view(-1) == state.long()).all()),
                        "torch_scores_equal": bool((tscore.view(torch.int64) == score.view(torch.int64)).all())}
                for k, v in ts.items():
                    line[k + "_ms"] = spread(v)
                emit(line)
                del z, z3, ext, skip


def cli_case(emit):
    import torch

    import align_phones
    import viterbi_ref

    c = viterbi_ref.corpus(500, 20, 16, 1.3, 0)
    ptr = np.concatenate([[0], np.cumsum(c["lengths"])])
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "feats.scp"), "w") as fs, open(os.path.join(tmp, "len.scp"), "w") as ls, open(os.path.join(tmp, "text"), "w") as tx:
            for u in range(500):
                key = "u%04d" % u
                np.save(os.path.join(tmp, key + ".npy"), c["x"][ptr[u]:ptr[u + 1]])
                fs.write("%s %s\n" % (key, os.path.join(tmp, key + ".npy")))
                ls.write("%s %d\n" % (key, c["lengths"][u]))
                tx.write(" ".join([key] + ["p%02d" % p for p in c["refs"][u]]) + "\n")
        times = []
        for r in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            code = align_phones.main(["--feat-scp", os.path.join(tmp, "feats.scp"), "--len-scp", os.path.join(tmp, "len.scp"), "--on", "feats",
                                      "--text", os.path.join(tmp, "text"), "--out", os.path.join(tmp, "out"), "--iters", "100", "--ctc-context", "2"])
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t) * 1e3)
        info = json.load(open(os.path.join(tmp, "out", "align.json")))
    emit({"case": "align_phones_cli", "exit": code, "utterances": 500, "frames": int(ptr[-1]), "phones": 20, "width": 16, "iters": 100,
          "context": 2, "wall_ms": spread(times), "aligned": info["aligned"], "tokens": info["tokens"], "iterations": info["iterations"],
          "mean_path_logprob_per_frame": info["mean_path_logprob_per_frame"]})


def main(argv=None):
    ap = argparse.ArgumentParser(description="Forced alignment against the nll-only CTC pass and batched torch ops; align_phones.py end to end")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_falign.jsonl"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=None, choices=["align", "cli"])
    args = ap.parse_args(argv)
    require_gpu("bench_falign")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.only is None:
        open(args.out, "w").close()  # (the sink appends: a whole run starts the file anew)
    emit = open_sink(args.out)
    if args.only in (None, "align"):
        align_cases(args.reps, emit)
    if args.only in (None, "cli"):
        cli_case(emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
