"""Times of the CTC prefix beam search (include/fhvae_ctcbeam.h) on one MI355X, against ctc.greedy's arg-max and collapse as torch
ops (the floor) and against the nll-only CTC pass on the same rows (the same sequential float64 structure), and of
ctcbeam.recognise end to end.

    python tools/bench_ctcbeam.py [--out profiles/bench_ctcbeam.jsonl] [--reps 5] [--only decode|recognise]

Cases (tools/bench_ctc.py's shapes): 1 h and 10 h of 10 ms frames as 10 s utterances, and 1 h as 60 s utterances, at C = 40 and
62 (the blank last), beam 1, 8 and 64, with a bigram table, at class_beam = inf and at class_beam = 8 (a class is extended into
when its probability is at least e^-8 of the frame's best).  Per case, alternated:
  hip_beam     ctcbeam.decode (the check kernel, the search, one read of status and lengths, the gather of the tokens)
  torch_greedy arg-max per row, phonerec.collapse, the blank dropped: what ctc.greedy does after its logits
  hip_ctc_nll  ctc.loss(..., want_grad=False) on the same rows with transcriptions of 90 to 110 (230 to 250) labels
  torchaudio   its CTC decoder, only if `import torchaudio` succeeds; otherwise the line says it is not installed
A line holds the median [min, max] in milliseconds of --reps device-event timings per side after one warm-up and the frames per
second of the search.  `recognise` fits a model on the generator's corpus and times ctcbeam.recognise (bigram, tuning grid on
the training utterances, search) on a host clock.  One JSON line per case; no speed is promised.
"""
import argparse
import os
import sys
import time

import numpy as np

from bench_common import ROOT, alternate, open_sink, require_gpu, spread

sys.path.insert(2, os.path.join(ROOT, "tests"))

CLASS_BEAM = 8.0


def decode_cases(reps, emit):
    import torch

    import ctc
    import ctcbeam
    import phonerec

    try:
        import torchaudio  # noqa: F401
        have_ta = True
    except Exception:  # noqa: BLE001
        have_ta = False
    dev = torch.device("cuda:0")
    for C in (40, 62):
        for name, U, T, lo, hi in (("1h_10s", 360, 1000, 90, 110), ("10h_10s", 3600, 1000, 90, 110), ("1h_60s", 60, 6000, 230, 250)):
            rng = np.random.default_rng(C + U)
            lens = rng.integers(lo, hi + 1, U)
            seqs = [rng.integers(0, C - 1, n) for n in lens]
            blank = C - 1
            flat = torch.from_numpy(np.concatenate(seqs).astype(np.int32)).to(dev)
            lab_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
            g = torch.Generator(device=dev).manual_seed(C + U)
            z = 3.0 * torch.randn(U * T, C, generator=g, device=dev)
            ptr = (torch.arange(U + 1, dtype=torch.int64) * T).to(dev)
            table = torch.from_numpy(ctcbeam.table(ctcbeam.bigram([s.tolist() for s in seqs], C, blank), 1.0, 0.0)).to(dev)
            ident = np.arange(C, dtype=np.int32)
            ident[blank] = -1

            def greedy():
                return phonerec.fold(*phonerec.collapse(torch.argmax(z, dim=1).to(torch.int32), ptr), ident)

            for W in (1, 8, 64):
                for class_beam in (float("inf"), CLASS_BEAM):
                    fns = {"hip_beam": lambda: ctcbeam.decode(z, ptr, blank, W, table, class_beam),
                           "torch_greedy": greedy,
                           "hip_ctc_nll": lambda: ctc.loss(z, ptr, flat, lab_ptr, blank, want_grad=False)}
                    ts = alternate(fns, reps)
                    tokens, hp, score, bits = ctcbeam.decode(z, ptr, blank, W, table, class_beam, with_status=True)
                    sec = np.median(ts["hip_beam"]) * 1e-3
                    line = {"case": "ctcbeam_" + name, "C": C, "beam": W, "class_beam": class_beam if class_beam != float("inf") else "inf",
                            "utterances": U, "frames": U * T, "status": int(bits), "tokens": int(tokens.shape[0]),
                            "greedy_tokens": int(greedy()[0].shape[0]), "frames_per_s": U * T / sec,
                            "us_per_frame_of_an_utterance": sec * 1e6 / T,
                            "torchaudio": "not installed" if not have_ta else "installed, not timed"}
                    for k, v in ts.items():
                        line[k + "_ms"] = spread(v)
                    emit(line)
            del z


def recognise_case(emit):
    import torch

    import ctc
    import ctcbeam
    import viterbi_ref

    c = viterbi_ref.corpus(500, 20, 16, 1.3, 0)
    ptr = np.concatenate([[0], np.cumsum(c["lengths"])])
    cut = int(ptr[400])
    dev = torch.device("cuda:0")
    train_x, test_x = torch.from_numpy(c["x"][:cut]).to(dev), torch.from_numpy(c["x"][cut:]).to(dev)
    lens, names = c["lengths"], ["p%02d" % i for i in range(20)]
    t = time.perf_counter()
    model, greedy, _, _ = ctc.recognise(train_x, lens[:400], c["refs"][:400], test_x, lens[400:], c["refs"][400:], names, iters=100, context=2)
    torch.cuda.synchronize()
    fit_ms = (time.perf_counter() - t) * 1e3
    times, rep = [], None
    for r in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        rep = ctcbeam.recognise(train_x, lens[:400], c["refs"][:400], test_x, lens[400:], c["refs"][400:], names, beam=16, model=model)[1]
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    fixed = ctcbeam.recognise(train_x, lens[:400], c["refs"][:400], test_x, lens[400:], c["refs"][400:], names, beam=16, scale=1.0, bonus=0.0,
                              model=model)[1]
    emit({"case": "ctcbeam_recognise", "utterances": 500, "train": 400, "frames": int(ptr[-1]), "phones": 20, "width": 16, "iters": 100,
          "context": 2, "beam": 16, "grid_points": len(rep["grid"]), "ctc_recognise_with_fit_ms": fit_ms, "wall_ms": spread(times),
          "per_greedy": greedy["per"], "per_beam_tuned": rep["per"], "lm_scale": rep["lm_scale"], "bonus": rep["bonus"],
          "per_beam_scale1_bonus0": fixed["per"], "train_per_grid": rep["grid"]})


def main(argv=None):
    ap = argparse.ArgumentParser(description="CTC prefix beam search against torch's greedy decode and the nll-only CTC pass; ctcbeam.recognise end to end")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_ctcbeam.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, choices=["decode", "recognise"])
    args = ap.parse_args(argv)
    require_gpu("bench_ctcbeam")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.only is None:
        open(args.out, "w").close()  # (the sink appends: a whole run starts the file anew)
    emit = open_sink(args.out)
    if args.only in (None, "decode"):
        decode_cases(args.reps, emit)
    if args.only in (None, "recognise"):
        recognise_case(emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
