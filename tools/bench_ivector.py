"""i-vector extraction on one MI355X (csrc/ivector.hip, ivector.py) -- prints one JSON line per measurement.

  stats   fhvae_iv_stats on random rows and posteriors: 1 h and 10 h of frames (360 000 per hour) as 10 s utterances, 1 h as one
          utterance, C = 256 / 2048, width 39 / 60.  Beside gmm.accumulate (fhvae_gmm_stats) on the same rows -- the same product
          without the segmentation, plus the squares -- and beside torch ops: bmm of post^T . x per utterance (one matrix product
          for the single utterance), plus the sum of post.
  solve   fhvae_iv_solve (w, E, logdet) at R = 32 / 64 / 128, U = 360 / 28 000, beside torch.linalg.cholesky + cholesky_solve +
          cholesky_inverse (+ the outer product and the log-determinant) in float64 on the unpacked matrices.
  em      one EM iteration with minimum divergence and one extract at 10 h of 10 s utterances, C = 2048, width 39, R = 128, split
          by host clock with a device sync after each part: statistics (utterance_stats: loglik, posteriors, stats), whitening,
          the E-steps' matrix products, solve, the M-step's sums, host algebra (M_c, the C solves, G).
  cli     extract_ivectors.py end to end on a generated archive: 1 h of 10 s utterances, C = 256, width 39, R = 64.

Alternated runs, median [min, max] (tools/bench_common.py).

    python tools/bench_ivector.py [--reps 7] [--only stats solve em cli] [--out FILE.jsonl]
"""
import argparse
import time

import numpy as np

import bench_common as BC

FRAMES_PER_HOUR = 360000


def ms(ts, name):
    s = BC.spread(ts[name])
    return {name + "_ms_median": round(s["median"], 3), name + "_ms_min": round(s["min"], 3), name + "_ms_max": round(s["max"], 3)}


def random_post(N, C, dev, seed):
    import torch

    g = torch.Generator(device=dev).manual_seed(seed)
    post = torch.empty(N, C, dtype=torch.float32, device=dev)
    step = max(1, (1 << 28) // C)
    for a in range(0, N, step):  # (in row chunks: no second (N, C) array)
        z = torch.randn(min(step, N - a), C, generator=g, device=dev) * 3.0
        post[a:a + step] = torch.softmax(z, dim=1)
    return post


def bench_stats(emit, hours, utt_frames, C, width, reps):
    import torch

    import gmm
    import ivector

    dev = torch.device("cuda")
    N = int(hours * FRAMES_PER_HOUR)
    utt_frames = N if utt_frames is None else utt_frames
    U = N // utt_frames
    Dp = ivector.padded(width)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.zeros(N, Dp, device=dev)
    x[:, :width] = torch.randn(N, width, generator=g, device=dev)
    post = random_post(N, C, dev, 2)
    ptr = torch.arange(U + 1, dtype=torch.int64, device=dev) * utt_frames
    status = ivector.hip_ext.status_word(dev)
    ones = torch.ones(utt_frames, 1, device=dev)

    def k_iv():
        ivector.stats(x, post, ptr, status=status)

    def k_gmm():
        gmm.accumulate(x, post)

    def t_bmm():
        pt = post.view(U, utt_frames, C).transpose(1, 2)
        torch.bmm(pt, x.view(U, utt_frames, Dp))
        pt @ ones

    ts = BC.alternate({"iv_stats": k_iv, "gmm_stats": k_gmm, "torch_bmm": t_bmm}, reps)
    assert int(status.item()) == 0
    res = {"bench": "iv_stats", "hours": hours, "utterances": U, "frames": N, "C": C, "width": width, "reps": reps}
    for name in ts:
        res.update(ms(ts, name))
    res["flop"] = 2.0 * N * C * (Dp + 1)
    emit(res)


def bench_solve(emit, R, U, reps):
    import torch

    import ivector

    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(R)
    A = torch.randn(U, R, R + 8, dtype=torch.float64, generator=g, device=dev)
    L = torch.eye(R, dtype=torch.float64, device=dev)[None] + A @ A.transpose(1, 2)
    del A
    b = torch.randn(U, R, dtype=torch.float64, generator=g, device=dev)
    Lp = ivector.pack(L)
    status = ivector.hip_ext.status_word(dev)

    def k_solve():
        ivector.solve(Lp, b, status=status)

    def k_w():
        ivector.solve(Lp, b, want_E=False, want_logdet=False, status=status)

    def t_chol():
        G = torch.linalg.cholesky(L)
        w = torch.cholesky_solve(b[:, :, None], G)[:, :, 0]
        E = torch.cholesky_inverse(G) + w[:, :, None] * w[:, None, :]
        ld = 2.0 * torch.log(torch.diagonal(G, dim1=1, dim2=2)).sum(dim=1)
        return w, E, ld

    ts = BC.alternate({"iv_solve": k_solve, "iv_solve_w_only": k_w, "torch_cholesky": t_chol}, {"iv_solve": reps, "iv_solve_w_only": reps, "torch_cholesky": min(reps, 3)})
    assert int(status.item()) == 0
    res = {"bench": "iv_solve", "R": R, "U": U, "reps": reps}
    for name in ts:
        res.update(ms(ts, name))
    emit(res)


def bench_em(emit, hours, C, width, R):
    import torch

    import ivector

    dev = torch.device("cuda")
    N, utt = int(hours * FRAMES_PER_HOUR), 1000
    U = N // utt
    rng = np.random.default_rng(0)
    ubm = {"weights": np.full(C, 1.0 / C), "means": rng.standard_normal((C, width)) * 2.0, "variances": 0.5 + rng.random((C, width))}
    g = torch.Generator(device=dev).manual_seed(3)
    rows = torch.randn(N, width, generator=g, device=dev) * 2.0
    ptr = np.arange(U + 1, dtype=np.int64) * utt
    parts = {}

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        parts[name] = parts.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
        return out

    n, f = timed("statistics", lambda: ivector.utterance_stats(rows, ptr, ubm))
    n, f = None, None
    parts.clear()
    n, f = timed("statistics", lambda: ivector.utterance_stats(rows, ptr, ubm))
    ft = timed("whiten", lambda: ivector.whiten(n, f, ubm))
    Dp = ivector.padded(width)
    T = np.zeros((C, Dp, R))
    T[:, :width] = 0.1 * rng.standard_normal((C, width, R))
    T = T.reshape(C * Dp, R)
    nd = n.double()
    status = ivector.hip_ext.status_word(dev)
    P = R * (R + 1) // 2

    def estep(T, sums):
        M = timed("host", lambda: torch.from_numpy(ivector._gram(T, C, Dp)).to(dev))
        Td = torch.from_numpy(T).to(dev)
        eye = torch.from_numpy(ivector.pack(np.eye(R))).to(dev)
        A = torch.zeros(C, P, dtype=torch.float64, device=dev)
        K = torch.zeros(C * Dp, R, dtype=torch.float64, device=dev)
        Es = torch.zeros(P, dtype=torch.float64, device=dev)
        step = ivector._utt_chunk(U, R, 1 << 30)
        for a in range(0, U, step):
            b = min(U, a + step)
            Lp, bu = timed("products", lambda: ((nd[a:b] @ M + eye[None]).contiguous(), (ft[a:b] @ Td).contiguous()))
            w, E, ld = timed("solve", lambda: ivector.solve(Lp, bu, status=status))
            if sums:
                timed("sums", lambda: (A.add_(nd[a:b].t() @ E), K.add_(ft[a:b].t() @ w), Es.add_(E.sum(dim=0))))
        return A, K, Es

    A, K, Es = estep(T, True)

    def host_m():
        Ah, Kh = ivector.unpack(A.cpu().numpy(), R), K.cpu().numpy().reshape(C, Dp, R)
        return np.stack([np.linalg.solve(Ah[c], Kh[c].T).T for c in range(C)]).reshape(C * Dp, R)

    T = timed("host", host_m)
    _, _, Es = estep(T, True)
    T = timed("host", lambda: T @ np.linalg.cholesky(ivector.unpack(Es.cpu().numpy() / U, R)))
    res = {"bench": "iv_em_iteration", "hours": hours, "utterances": U, "C": C, "width": width, "R": R}
    res.update({k + "_ms": round(v, 1) for k, v in parts.items()})
    emit(res)
    model = {"T": T, "means": ubm["means"], "variances": ubm["variances"]}
    parts.clear()
    timed("extract", lambda: ivector.extract(n, f, model))
    emit({"bench": "iv_extract", "hours": hours, "utterances": U, "C": C, "width": width, "R": R, "extract_ms": round(parts["extract"], 1)})


def bench_cli(emit, hours, C, width, R):
    """extract_ivectors.py end to end (host clock) on a generated numpy archive of 10 s utterances: the archive read, a UBM fitted
    (5 iterations), the statistics, 2 EM iterations, the extraction, the files written."""
    import os
    import tempfile

    import extract_ivectors as EI

    rng = np.random.default_rng(1)
    U = int(hours * FRAMES_PER_HOUR) // 1000
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "feats.scp"), "w") as fs, open(os.path.join(d, "len.scp"), "w") as ls:
            for u in range(U):
                path = os.path.join(d, "u%05d.npy" % u)
                np.save(path, (rng.standard_normal((1000, width)) * 2.0 + rng.standard_normal(width)).astype(np.float32))
                fs.write("spk%03d-u%05d %s\n" % (u % 40, u, path))
                ls.write("spk%03d-u%05d 1000\n" % (u % 40, u))
        argv = ["--feat-scp", os.path.join(d, "feats.scp"), "--len-scp", os.path.join(d, "len.scp"), "--ubm-k", str(C), "--ubm-iters", "5",
                "--rank", str(R), "--iters", "2", "--out", os.path.join(d, "out")]
        t0 = time.perf_counter()
        rc = EI.main(argv)
        dt = time.perf_counter() - t0
    assert rc == 0
    emit({"bench": "extract_ivectors_cli", "hours": hours, "utterances": U, "C": C, "width": width, "R": R, "ubm_iters": 5, "iters": 2,
          "seconds": round(dt, 2)})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", nargs="+", default=["stats", "solve", "em", "cli"], choices=["stats", "solve", "em", "cli"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    BC.require_gpu("bench_ivector.py")
    emit = BC.open_sink(args.out)
    if "stats" in args.only:
        for C in (256, 2048):
            for width in (39, 60):
                for hours, utt in ((1, 1000), (10, 1000), (1, None)):
                    bench_stats(emit, hours, utt, C, width, args.reps)
    if "solve" in args.only:
        for R in (32, 64, 128):
            for U in (360, 28000):
                bench_solve(emit, R, U, args.reps)
    if "em" in args.only:
        bench_em(emit, 10, 2048, 39, 128)
    if "cli" in args.only:
        bench_cli(emit, 1, 256, 39, 64)


if __name__ == "__main__":
    main()
