"""Energy VAD on one MI355X (csrc/vad.hip, pytorch-scalablefhvae_amd/vad.py) -- one JSON line per measurement.

  kernels  fhvae_vad_energy (centred RMS, 400 / 160 samples at 16 kHz), fhvae_vad_decide (the reference's convention) and
           fhvae_vad_select (F = 80) over 1 min, 10 min and 1 h of 16 kHz audio in 10 s utterances, and 1 h as one utterance,
           the whole corpus in one call, each against the same step as torch ops: the energy as a float64 cumsum of the
           squared, reflect-padded samples differenced at the frame edges; the decision as segment_reduce, repeat_interleave
           and a comparison, the rank as a cumsum; the selection as boolean indexing.  Both paths of a case alternate, 10
           runs each, device events around every run: median [min, max] ms.  For the energy: the bytes it must move (the
           samples once + the energies written) per second of the median against the 8 TB/s HBM peak, and fhvae_feats_fwd
           (80 mel bins) on the same batch in the same alternation.  Whether both paths decide alike is reported.
  cli      prepare_numpy_data.py over a generated corpus (10 s WAV files) with --vad drop against the same run without the
           flag, alternated, host clock.

    python tools/bench_vad.py [--reps 10] [--minutes 1 10 60] [--cli-minutes 60] [--cli-reps 3] [--out profiles/bench_vad.jsonl]
"""
import argparse
import os
import shutil
import tempfile
import time

import numpy as np

from bench_common import alternate, open_sink, require_gpu, spread  # (importing it sets the package's import path)

PEAK_HBM = 8.0e12
SR, L, HOP, F = 16000, 400, 160, 80
UTT = 10 * SR
TH_RATIO = 1.04 / 2


def signal(n, seed):
    """Gaussian noise whose amplitude alternates between 0.3 and 0.003 every 0.1 s (the tests' signal)."""
    rng = np.random.default_rng(seed)
    amp = np.where((np.arange(n) // (SR // 10)) % 2 == 0, np.float32(0.3), np.float32(0.003))
    return rng.standard_normal(n, dtype=np.float32) * amp


def torch_energy(wave2d):
    """(U, n) equal-length utterances -> (U * frames,) centred RMS, float64 inside, as torch ops without unfold."""
    import torch

    p = torch.nn.functional.pad(wave2d.unsqueeze(1), (L // 2, L // 2), mode="reflect").squeeze(1).double()
    cs = torch.nn.functional.pad(torch.cumsum(p * p, dim=1), (1, 0))
    frames = 1 + (wave2d.shape[1] + 2 * (L // 2) - L) // HOP
    a = torch.arange(frames, device=wave2d.device) * HOP
    return torch.sqrt((cs[:, a + L] - cs[:, a]) / L).float().reshape(-1)


def torch_decide(energy, lengths_d):
    import torch

    e = energy.double()
    th = TH_RATIO * torch.segment_reduce(e, "sum", lengths=lengths_d) / lengths_d
    vad = e > torch.repeat_interleave(th, lengths_d, output_size=e.shape[0])
    rank = torch.nn.functional.pad(torch.cumsum(vad, 0), (1, 0))
    return vad, rank


def bench_kernels(minutes, one_utterance, reps, emit):
    import torch

    import features as FT
    import hip_binding as hb
    import vad as V

    n = minutes * 60 * SR
    U = 1 if one_utterance else n // UTT
    wave = torch.from_numpy(signal(n, minutes)).cuda()
    lens = np.full(U, n // U, dtype=np.int64)
    frames = FT.num_frames(lens, L, HOP)
    wave_ptr, frame_ptr = FT._ptr(lens), FT._ptr(frames)
    N = int(frame_ptr[-1])
    ptrs = torch.from_numpy(np.stack([wave_ptr, frame_ptr])).cuda()
    lengths_d = torch.from_numpy(frames).cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    bases = FT._Bases(SR, L, F, "fbank", "cuda")
    feats = torch.empty((N, F), dtype=torch.float32, device="cuda")
    base = {"audio_min": minutes, "utterances": U, "samples": n, "frames": N, "frame_len": L, "hop": HOP, "reps": reps}
    keep = {}

    def k_energy():
        keep["ke"] = V.energy(wave, ptrs[0], ptrs[1], N, L, HOP, V.VAD_RMS_CENTER, 0, status)

    def t_energy():
        keep["te"] = torch_energy(wave.view(U, -1))

    def k_feats():
        hb.feats_fwd(wave, ptrs[0], ptrs[1], bases.dft, bases.mel, L, HOP, F, "fbank", feats, status)

    ts = alternate({"kernel": k_energy, "torch": t_energy, "feats_fwd": k_feats}, reps, warmup=2)
    rel = float(((keep["ke"].double() - keep["te"].double()).abs() / keep["te"].double().abs().clamp_min(1e-30)).max())
    need = 4.0 * (n + N)
    mk = float(np.median(ts["kernel"]))
    emit(dict(base, bench="vad_energy", ms_kernel=spread(ts["kernel"]), ms_torch=spread(ts["torch"]), ms_feats_fwd=spread(ts["feats_fwd"]),
              torch_over_kernel=float(np.median(ts["torch"])) / mk, kernel_over_feats_fwd=mk / float(np.median(ts["feats_fwd"])),
              bytes_needed=need, kernel_bytes_per_s=need / (mk * 1e-3), kernel_hbm_fraction=need / (mk * 1e-3) / PEAK_HBM,
              max_rel_diff_vs_torch=rel))
    energy = keep["ke"]
    del keep["te"]
    torch.cuda.empty_cache()

    def k_decide():
        keep["kd"] = V.decide(energy, ptrs[1], 0.0, TH_RATIO, 0, 1.0, status)

    def t_decide():
        keep["td"] = torch_decide(energy, lengths_d)

    ts = alternate({"kernel": k_decide, "torch": t_decide}, reps, warmup=2)
    same = bool(torch.equal(keep["kd"][0].bool(), keep["td"][0]) and torch.equal(keep["kd"][1], keep["td"][1]))
    mk = float(np.median(ts["kernel"]))
    vad, rank = keep["kd"]
    n_out = int(rank[-1].item())
    emit(dict(base, bench="vad_decide", ms_kernel=spread(ts["kernel"]), ms_torch=spread(ts["torch"]),
              torch_over_kernel=float(np.median(ts["torch"])) / mk, voiced=n_out, same_decisions_and_rank=same))
    feats.normal_()
    mask = keep["td"][0]

    def k_select():
        keep["ks"] = V.select(feats, vad, rank, n_out, status)

    def t_select():
        keep["ts"] = feats[mask]

    ts = alternate({"kernel": k_select, "torch": t_select}, reps, warmup=2)
    same = bool(torch.equal(keep["ks"].view(torch.int32), keep["ts"].view(torch.int32)))
    need = 4.0 * F * 2 * n_out
    mk = float(np.median(ts["kernel"]))
    emit(dict(base, bench="vad_select", F=F, rows_out=n_out, ms_kernel=spread(ts["kernel"]), ms_torch=spread(ts["torch"]),
              torch_over_kernel=float(np.median(ts["torch"])) / mk, bytes_needed=need, kernel_bytes_per_s=need / (mk * 1e-3),
              same_bits=same))
    assert int(status.item()) == 0


def bench_cli(minutes, reps, emit):
    import features as FT
    import prepare_numpy_data as PN

    d = tempfile.mkdtemp(prefix="bench_vad_")
    try:
        os.makedirs(os.path.join(d, "train"))
        U = minutes * 6
        with open(os.path.join(d, "train", "wav.scp"), "w") as scp:
            for j in range(U):
                path = os.path.join(d, "u%04d.wav" % j)
                FT.write_wav(path, np.clip(signal(UTT, j), -0.999, 0.999), SR)
                scp.write("u%04d %s\n" % (j, path))
        wall = {"plain": [], "vad_drop": []}
        for r in range(reps + 1):  # (the first round warms the file cache and the device up)
            for name, vad in (("plain", None), ("vad_drop", "drop")):
                out = os.path.join(d, "np_%s" % name)
                t, t0 = {}, time.perf_counter()
                PN.prepare_numpy("librispeech", "train", d, out, timings=t, vad=vad)
                dt = time.perf_counter() - t0
                if r:
                    wall[name].append(dict(t, total=dt))
                shutil.rmtree(out)
        med = {k: {p: float(np.median([w[p] for w in v])) for p in ("read", "gpu", "write", "total")} for k, v in wall.items()}
        emit({"bench": "prepare_numpy_data", "audio_min": minutes, "files": U, "reps": reps, "seconds_median": med,
              "vad_drop_over_plain_total": med["vad_drop"]["total"] / med["plain"]["total"],
              "vad_drop_over_plain_gpu": med["vad_drop"]["gpu"] / med["plain"]["gpu"]})
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

    require_gpu("bench_vad.py")
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
