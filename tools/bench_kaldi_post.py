"""Cepstra, deltas and sliding CMVN on one MI355X (csrc/kaldi_post.hip, pytorch-scalablefhvae_amd/kaldi_post.py) -- one JSON
line per measurement.

  kernels  fhvae_kaldi_cepstra (B = 23 -> 13 and 80 -> 40, with the lifter), fhvae_kaldi_add_deltas (D = 13 and 80, order 2,
           window 2) and fhvae_kaldi_cmvn_sliding (D = 39, window 300, centred, mean only) over 1 min, 10 min and 1 h of
           frames at 100 per second in 10 s utterances, and 1 h as one utterance, the whole corpus in one call, each against
           the same step as torch ops: the cepstra as a matmul and a scale; the deltas as replicate-pad plus conv1d per
           utterance (the equal-length utterances as one batch); the CMVN as a float64 cumsum differenced at the window
           edges.  Both paths of a case alternate, 10 runs each, device events around every run: median [min, max] ms, and
           the bytes the step must move (its input once + its output once) per second of the median against the 8 TB/s HBM
           peak.  The largest difference between the two paths is reported.
  cli      prepare_kaldi_data.py over a generated corpus (10 s WAV files): --mfcc_conf --add-deltas --cmvn-sliding against
           the plain fbank run, alternated, host clock.

    python tools/bench_kaldi_post.py [--reps 10] [--minutes 1 10 60] [--cli-minutes 60] [--cli-reps 3] [--out profiles/bench_kaldi_post.jsonl]
"""
import argparse
import os
import shutil
import tempfile
import time

import numpy as np

from bench_common import alternate, open_sink, require_gpu, spread  # (importing it sets the package's import path)

PEAK_HBM = 8.0e12
SR, FPS = 16000, 100
UTT_FRAMES = 10 * FPS
CMN_WINDOW = 300


def torch_deltas(x3, kernels, order, window):
    """(U, T, D) equal-length utterances -> (U, T, (order + 1) D): replicate-pad and a depthwise conv1d per order."""
    import torch

    U, T, D = x3.shape
    rows = x3.transpose(1, 2).reshape(U * D, 1, T)
    out = [x3]
    for i in range(1, order + 1):
        p = torch.nn.functional.pad(rows, (i * window, i * window), mode="replicate")
        out.append(torch.nn.functional.conv1d(p, kernels[i]).reshape(U, D, T).transpose(1, 2))
    return torch.cat(out, dim=2)


def torch_cmvn(x3, b, e):
    """(U, T, D) -> x less the mean over [b[t], e[t]) of its utterance: float64 cumsum differenced at the window edges."""
    import torch

    cs = torch.nn.functional.pad(torch.cumsum(x3.double(), dim=1), (0, 0, 1, 0))
    mean = (cs[:, e] - cs[:, b]) / (e - b).double()[None, :, None]
    return (x3.double() - mean).float()


def report(emit, base, bench, ts, need, diff, **more):
    mk = float(np.median(ts["kernel"]))
    emit(dict(base, bench=bench, ms_kernel=spread(ts["kernel"]), ms_torch=spread(ts["torch"]),
              torch_over_kernel=float(np.median(ts["torch"])) / mk, bytes_needed=need, kernel_bytes_per_s=need / (mk * 1e-3),
              kernel_hbm_fraction=need / (mk * 1e-3) / PEAK_HBM, max_abs_diff_vs_torch=diff, **more))


def bench_kernels(minutes, one_utterance, reps, emit):
    import torch

    import kaldi_post as KP

    n = minutes * 60 * FPS
    U = 1 if one_utterance else n // UTT_FRAMES
    T = n // U
    ptr = torch.arange(U + 1, dtype=torch.int64, device="cuda") * T
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    base = {"audio_min": minutes, "utterances": U, "frames": n, "reps": reps}
    gen = torch.Generator(device="cuda").manual_seed(minutes)
    keep = {}
    for B, C in ((23, 13), (80, 40)):
        m = torch.randn((n, B), device="cuda", generator=gen) * 4.0 + 8.0
        dct, lf = torch.from_numpy(KP.dct_matrix(C, B)).cuda(), torch.from_numpy(KP.lifter_coeffs(C, 22.0)).cuda()
        dct_t = dct.t().contiguous()

        def k_cep():
            keep["k"] = KP.cepstra(m, dct, lf)

        def t_cep():
            keep["t"] = (m @ dct_t) * lf

        ts = alternate({"kernel": k_cep, "torch": t_cep}, reps, warmup=2)
        report(emit, base, "kaldi_cepstra", ts, 4.0 * n * (B + C), float((keep["k"] - keep["t"]).abs().max()), B=B, C=C)
        del m
        keep.clear()
        torch.cuda.empty_cache()
    for D in (13, 80):
        x = torch.randn((n, D), device="cuda", generator=gen)
        kernels = [None] + [torch.from_numpy(s).cuda().view(1, 1, -1) for s in KP.delta_scales(2, 2)[1:]]

        def k_del():
            keep["k"] = KP.add_deltas(x, ptr, 2, 2, status)

        def t_del():
            keep["t"] = torch_deltas(x.view(U, T, D), kernels, 2, 2)

        ts = alternate({"kernel": k_del, "torch": t_del}, reps, warmup=2)
        report(emit, base, "kaldi_add_deltas", ts, 4.0 * n * D * 4, float((keep["k"] - keep["t"].reshape(n, 3 * D)).abs().max()), D=D,
               order=2, window=2)
        del x
        keep.clear()
        torch.cuda.empty_cache()
    D = 39
    x = torch.randn((n, D), device="cuda", generator=gen) * 3.0 + 5.0
    win = np.array([KP.cmvn_window(t, T, CMN_WINDOW, 100, True) for t in range(T)], dtype=np.int64)
    b, e = torch.from_numpy(win[:, 0].copy()).cuda(), torch.from_numpy(win[:, 1].copy()).cuda()

    def k_cmvn():
        keep["k"] = KP.cmvn_sliding(x, ptr, CMN_WINDOW, 100, True, False, status)

    def t_cmvn():
        keep["t"] = torch_cmvn(x.view(U, T, D), b, e)

    ts = alternate({"kernel": k_cmvn, "torch": t_cmvn}, reps, warmup=2)
    report(emit, base, "kaldi_cmvn_sliding", ts, 4.0 * n * D * 2, float((keep["k"] - keep["t"].reshape(n, D)).abs().max()), D=D,
           cmn_window=CMN_WINDOW, center=True, norm_vars=False)
    assert int(status.item()) == 0


def bench_cli(minutes, reps, emit):
    import features as FT
    import prepare_kaldi_data as PK

    d = tempfile.mkdtemp(prefix="bench_kaldi_post_")
    try:
        os.makedirs(os.path.join(d, "train"))
        U = minutes * 6
        with open(os.path.join(d, "train", "wav.scp"), "w") as scp:
            for j in range(U):
                path = os.path.join(d, "u%04d.wav" % j)
                rng = np.random.default_rng(j)
                amp = np.where((np.arange(10 * SR) // (SR // 10)) % 2 == 0, np.float32(0.3), np.float32(0.003))
                FT.write_wav(path, np.clip(rng.standard_normal(10 * SR, dtype=np.float32) * amp, -0.999, 0.999), SR)
                scp.write("u%04d %s\n" % (j, path))
        fbank, mfcc = os.path.join(d, "fbank.conf"), os.path.join(d, "mfcc.conf")
        open(fbank, "w").write("--num-mel-bins=80\n")
        open(mfcc, "w").write("--num-ceps=13\n")
        import kaldi_post as KP

        runs = {"fbank": dict(fbank_conf=fbank), "mfcc_deltas_cmvn": dict(mfcc_conf=mfcc, deltas=KP.deltas_spec(), cmvn=KP.cmvn_spec())}
        wall = {k: [] for k in runs}
        for r in range(reps + 1):  # (the first round warms the file cache and the device up)
            for name, kw in runs.items():
                t, t0 = {}, time.perf_counter()
                PK.prepare_kaldi(d, "train", timings=t, **kw)
                dt = time.perf_counter() - t0
                if r:
                    wall[name].append(dict(t, total=dt))
        med = {k: {p: float(np.median([w[p] for w in v])) for p in ("read", "gpu", "write", "total")} for k, v in wall.items()}
        emit({"bench": "prepare_kaldi_data", "audio_min": minutes, "files": U, "reps": reps, "seconds_median": med,
              "mfcc_over_fbank_total": med["mfcc_deltas_cmvn"]["total"] / med["fbank"]["total"],
              "mfcc_over_fbank_gpu": med["mfcc_deltas_cmvn"]["gpu"] / med["fbank"]["gpu"]})
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--minutes", type=int, nargs="*", default=[1, 10, 60])
    ap.add_argument("--one-utterance-minutes", type=int, nargs="*", default=[60])
    ap.add_argument("--cli-minutes", type=int, nargs="*", default=[60])
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch

    require_gpu("bench_kaldi_post.py")
    emit = open_sink(args.out)

    for minutes in args.minutes:
        bench_kernels(minutes, False, args.reps, emit)
        torch.cuda.empty_cache()
    for minutes in args.one_utterance_minutes:
        bench_kernels(minutes, True, args.reps, emit)
        torch.cuda.empty_cache()
    for minutes in args.cli_minutes:
        bench_cli(minutes, args.cli_reps, emit)


if __name__ == "__main__":
    main()
