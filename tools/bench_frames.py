"""The frame-level layer on one MI355X (csrc/frames.hip, pytorch-scalablefhvae_amd/frames.py) -- one JSON line per measurement.

  kernels  fhvae_frames_gather and fhvae_frames_overlap_mean over 1 min, 10 min and 1 h of 80-bin features (10 s utterances of
           998 frames, T = 20, shift 1 and shift 8; the overlap mean needs shift <= 10 and is measured at shift 1 and 8 too),
           the whole corpus in one call, against the same step as torch ops: the gather as index arithmetic (bucketize, clamp)
           and advanced indexing, the overlap mean as utils.overlap_mean per utterance.  Both paths of a case alternate, 10
           runs each, device events around every run: median [min, max] ms.  bytes: what the step must move at least (the
           pool once + the windows written; the windows once + the frames written) per second of the median against the
           8 TB/s HBM peak.  Whether both paths gave the same bits is reported, not assumed.
  model    encode_frames and convert_frames over the 1 h corpus with the c3 model (2 x 256 LSTM nets, z = 32) in bf16,
           alternated, 10 runs each, host clock around calls that end in their own synchronise; and, from one more
           encode_frames run under the op timer, the device time per library entry point and the share spent outside
           fhvae_lstm_seq_infer.

    python tools/bench_frames.py [--reps 10] [--minutes 1 10 60] [--model-minutes 60] [--out profiles/bench_frames.jsonl]
"""
import argparse
import time

import numpy as np

from bench_common import alternate, open_sink, require_gpu, spread  # (importing it sets the package's import path)

PEAK_HBM = 8.0e12
T, F, UTT = 20, 80, 998


def corpus(minutes, seed=0):
    rng = np.random.default_rng(seed)
    level = rng.uniform(-10, 6, size=(1, F))
    return [np.clip(level + rng.standard_normal((UTT, F)) * 2.0, -16, 12).astype(np.float32) for _ in range(max(1, minutes * 6))]


def torch_gather(pool, lo, hi):
    """Windows [lo, hi) of a frames.FramePool as torch ops."""
    import torch

    w = torch.arange(lo, hi, device=pool.pool.device)
    u = torch.bucketize(w, pool.win_ptr[1:], right=True)
    a = pool.utt_ptr[u]
    n = pool.utt_ptr[u + 1] - a
    p = ((w - pool.win_ptr[u]) * pool.shift - pool.T // 2).unsqueeze(1) + torch.arange(pool.T, device=w.device)
    p = torch.minimum(torch.clamp(p, min=0), (n - 1).unsqueeze(1))
    return (pool.pool[a.unsqueeze(1) + p] - pool.mean) * pool.inv_std


def torch_overlap(pool, seg):
    """The overlap mean of a frames.FramePool's windows as utils.overlap_mean per utterance: with the frames moved up by
    left = T // 2 window k covers [k shift, k shift + T), which is the layout that function puts back together."""
    import torch

    import utils

    left, out = pool.T // 2, []
    for (w0, w1), n in zip(zip(pool.win_ptr_host[:-1], pool.win_ptr_host[1:]), pool.lengths):
        full, covered = utils.overlap_mean(seg[int(w0):int(w1)], pool.T, pool.shift, int(n) + left)
        assert covered == int(n) + left
        out.append(full[left:])
    return torch.cat(out) * pool.std + pool.mean


def bench_kernels(minutes, shift, reps, emit):
    import torch

    import frames as FR

    feats = corpus(minutes, minutes)
    rng = np.random.default_rng(1)
    pool = FR.FramePool(feats, T, shift, rng.standard_normal(F).astype(np.float32), rng.uniform(0.5, 2.0, F), device="cuda")
    W, N = pool.num_windows, pool.num_frames
    base = {"feature_min": minutes, "utterances": pool.num_utts, "frames": N, "windows": W, "T": T, "F": F, "shift": shift, "reps": reps}
    keep = {}

    def k_gather():
        keep["k"] = pool.windows(0, W)

    def t_gather():
        keep["t"] = torch_gather(pool, 0, W)

    ts = alternate({"kernel": k_gather, "torch": t_gather}, reps, warmup=2)
    same = bool(torch.equal(keep["k"].view(torch.int32), keep["t"].view(torch.int32)))
    need = 4.0 * F * (N + W * T)
    mk = float(np.median(ts["kernel"]))
    emit(dict(base, bench="frames_gather", ms_kernel=spread(ts["kernel"]), ms_torch=spread(ts["torch"]),
              torch_over_kernel=float(np.median(ts["torch"])) / mk, bytes_needed=need, kernel_bytes_per_s=need / (mk * 1e-3),
              kernel_hbm_fraction=need / (mk * 1e-3) / PEAK_HBM, same_bits=same))
    keep.clear()
    if shift > FR.max_overlap_shift(T):
        pool.check()
        return
    seg = torch.randn(W, T, F, device="cuda")

    def k_overlap():
        keep["k"] = pool.overlap_mean(seg, 0, 0, N)

    def t_overlap():
        keep["t"] = torch_overlap(pool, seg)

    ts = alternate({"kernel": k_overlap, "torch": t_overlap}, reps, warmup=2)
    same = bool(torch.equal(keep["k"].view(torch.int32), keep["t"].view(torch.int32)))
    close = bool(torch.allclose(keep["k"], keep["t"], rtol=1e-6, atol=1e-6))
    need = 4.0 * F * (N + W * T)
    mk = float(np.median(ts["kernel"]))
    emit(dict(base, bench="frames_overlap_mean", ms_kernel=spread(ts["kernel"]), ms_torch=spread(ts["torch"]),
              torch_over_kernel=float(np.median(ts["torch"])) / mk, bytes_needed=need, kernel_bytes_per_s=need / (mk * 1e-3),
              kernel_hbm_fraction=need / (mk * 1e-3) / PEAK_HBM, same_bits=same, close=close))
    pool.check()


def bench_model(minutes, reps, emit, batch=16384):
    import torch

    import frames as FR
    import hip_binding as hb
    from fhvae import FHVAE

    H, D = 256, 32
    torch.manual_seed(0)
    model = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, compute_dtype="bf16").cuda().eval()
    feats = corpus(minutes, minutes)
    rng = np.random.default_rng(1)
    pool = FR.FramePool(feats, T, 1, rng.standard_normal(F).astype(np.float32), rng.uniform(0.5, 2.0, F), device="cuda")
    mu2 = torch.randn(pool.num_utts, D, device="cuda")
    fns = {"encode_frames": lambda: FR.encode_frames(model, pool, batch), "convert_frames": lambda: FR.convert_frames(model, pool, mu2, batch)}
    for fn in fns.values():
        fn()
    wall = {k: [] for k in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()  # (ends in pool.check(): a read of the status word, which waits for the device)
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    base = {"feature_min": minutes, "utterances": pool.num_utts, "frames": pool.num_frames, "windows": pool.num_windows, "T": T, "F": F,
            "shift": 1, "model": "c3 bf16 (2 x 256 LSTM nets, z = 32)", "batch_size": batch, "reps": reps, "lstm_status": hb.lstm_sync_status()}
    for name in fns:
        med = float(np.median(wall[name]))
        emit(dict(base, bench=name, ms=spread(wall[name]), windows_per_s=pool.num_windows / (med * 1e-3)))
    hb.OP_TIMER.enable()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    FR.encode_frames(model, pool, batch)
    e1.record()
    ops = hb.OP_TIMER.summary()
    hb.OP_TIMER.disable()
    total = e0.elapsed_time(e1)
    per_op = {k: round(v[1], 4) for k, v in sorted(ops.items(), key=lambda kv: -kv[1][1])}
    infer = ops.get("fhvae_lstm_seq_infer", (0, 0.0))[1]
    emit(dict(base, bench="encode_frames_op_times", ms_total_device=total, ms_per_entry_point=per_op, ms_lstm_seq_infer=infer,
              share_outside_lstm_seq_infer=1.0 - infer / total,
              share_frames_gather=ops.get("fhvae_frames_gather", (0, 0.0))[1] / total))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--minutes", type=int, nargs="*", default=[1, 10, 60])
    ap.add_argument("--shifts", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--model-minutes", type=int, nargs="*", default=[60])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch

    require_gpu("bench_frames.py")
    emit = open_sink(args.out)

    for minutes in args.minutes:
        for shift in args.shifts:
            bench_kernels(minutes, shift, args.reps, emit)
            torch.cuda.empty_cache()
    for minutes in args.model_minutes:
        bench_model(minutes, args.reps, emit)


if __name__ == "__main__":
    main()
