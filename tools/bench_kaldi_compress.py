"""Kaldi compressed-matrix codec on one MI355X (fhvae_kaldi_decompress / fhvae_kaldi_compress, csrc/kaldi_cm.hip) -- prints one
JSON line per measurement, for 1 min, 10 min and 1 h of 80-bin features (10 s utterances of 998 frames, CM), and for the 1 h as
ONE utterance of 359 280 frames (--long-minutes; the encoder's select runs one workgroup per utterance and 8 columns, so a
lone long utterance is its worst case):

  kernel: HIP-event time of one decode call and one encode call over the batch (alternated, each with its own pair of
          events), and the bytes each must move (decode: 1 B read + 4 B written per value; encode: 4 B read by each of the
          min/max, quantise and the four select passes + 1 B written) per second against the 8 TB/s HBM peak;
  host:   the same decode as numpy (kaldi_io_lite.decompress, what load_mat runs), wall time;
  pool:   wall time of datasets.ResidentSegmentPool over the compressed archive of the corpus and over the uncompressed
          archive of the same (host-decoded) matrices -- the parent's path and the baseline -- alternated, on local disk
          (the files are in the page cache after the warm-up: the difference is decode + host copies + H2D, not disk reads).

    python tools/bench_kaldi_compress.py [--reps 10] [--pool-reps 5] [--minutes 1 10 60] [--long-minutes 60]
"""
import argparse
import json
import os
import shutil
import tempfile
import time

import numpy as np

from bench_common import spread  # (importing it sets the package's import path)

PEAK_HBM = 8.0e12
F, UTT = 80, 998


def corpus(minutes, seed=0, one_utterance=False):
    """`minutes` of fbank-like features as 10 s utterances, or as one utterance of the same number of frames."""
    rng = np.random.default_rng(seed)
    U = max(1, minutes * 6)
    level = rng.uniform(-10, 6, size=(1, F))
    mats = [np.clip(level + rng.standard_normal((UTT, F)) * 2.0, -16, 12).astype(np.float32) for _ in range(U)]
    return [np.concatenate(mats)] if one_utterance else mats


def bench(minutes, reps, pool_reps, one_utterance=False):
    import torch

    import datasets as D
    import hip_binding as hb
    import kaldi_io_lite as K

    mats = corpus(minutes, minutes, one_utterance)
    U, rows = len(mats), len(mats[0])
    frames = U * rows
    dev = torch.device("cuda")
    feats = torch.from_numpy(np.concatenate(mats)).to(dev)
    desc, n_tiles, n_bytes = hb.kaldi_cm_descs(["CM"] * U, [rows] * U, F, np.arange(U) * rows)
    desc_d = torch.from_numpy(desc.view(np.uint8)).to(dev)
    payload = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty_like(feats)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def enc():
        hb.kaldi_compress(feats, desc_d, n_tiles, payload, status)

    def dec():
        hb.kaldi_decompress(payload, desc_d, n_tiles, out, status)

    for _ in range(3):
        enc(), dec()
    torch.cuda.synchronize()
    ts = {"enc": [], "dec": []}
    for _ in range(reps):
        for name, fn in (("enc", enc), ("dec", dec)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1))
    assert int(status.item()) == 0
    # the device codec against the host's on the first utterance
    got = desc_d.cpu().numpy().view(hb.KALDI_CM_DESC)
    tok, want = K.compress_mat(mats[0])
    size = K.payload_size("CM", rows, F)
    first = payload[:size].cpu().numpy().tobytes()
    bitwise = first == want and np.array_equal(out[:rows].cpu().numpy(), K.decompress("CM", got["min_value"][0], got["range"][0], rows, F, first))
    vals = frames * F
    med = {k: float(np.median(v)) for k, v in ts.items()}
    blobs = payload.cpu().numpy()
    host_ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        for j in range(U):
            off = int(desc["payload_off"][j])
            K.decompress("CM", got["min_value"][j], got["range"][j], rows, F, blobs[off:off + size].tobytes())
        host_ts.append(time.perf_counter() - t0)
    res = {"bench": "kaldi_cm_kernels", "feature_min": minutes, "utterances": U, "rows_per_utterance": rows, "frames": frames, "reps": reps,
           "ms_decode": spread(ts["dec"]), "ms_encode": spread(ts["enc"]),
           "decode_bytes_per_s": 5.0 * vals / (med["dec"] * 1e-3), "decode_hbm_fraction": 5.0 * vals / (med["dec"] * 1e-3) / PEAK_HBM,
           "encode_bytes_per_s": 25.0 * vals / (med["enc"] * 1e-3), "encode_hbm_fraction": 25.0 * vals / (med["enc"] * 1e-3) / PEAK_HBM,
           "s_decode_numpy_host": spread(host_ts), "device_equals_host": bool(bitwise)}
    print(json.dumps(res), flush=True)

    tmp = tempfile.mkdtemp(prefix="kaldi_cm_")
    try:
        items = [("u%05d" % j, m) for j, m in enumerate(mats)]
        dirs = {}
        for mode in ("compressed", "uncompressed"):
            d = os.path.join(tmp, mode)
            os.makedirs(d)
            K.write_len_scp(os.path.join(d, "len.scp"), [(k, len(m)) for k, m in items])
            dirs[mode] = d
        K.write_ark_scp(os.path.join(dirs["compressed"], "feats.ark"), os.path.join(dirs["compressed"], "feats.scp"), items, compress="auto")
        K.write_ark_scp(os.path.join(dirs["uncompressed"], "feats.ark"), os.path.join(dirs["uncompressed"], "feats.scp"),
                        K.read_ark(os.path.join(dirs["compressed"], "feats.ark")))
        sets = {m: D.KaldiDataset(os.path.join(d, "feats.scp"), os.path.join(d, "len.scp"), min_len=20, mvn_path=None, seg_len=20, seg_shift=8)
                for m, d in dirs.items()}
        pools = {m: D.ResidentSegmentPool(ds) for m, ds in sets.items()}  # warm-up
        same = bool(torch.equal(pools["compressed"].pool.view(torch.int32), pools["uncompressed"].pool.view(torch.int32)))
        del pools
        wall = {m: [] for m in sets}
        for _ in range(pool_reps):
            for m, ds in sets.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                p = D.ResidentSegmentPool(ds)
                torch.cuda.synchronize()
                wall[m].append(time.perf_counter() - t0)
                del p
        mc, mu = float(np.median(wall["compressed"])), float(np.median(wall["uncompressed"]))
        print(json.dumps({"bench": "resident_pool_build", "feature_min": minutes, "utterances": U, "rows_per_utterance": rows, "frames": frames, "reps": pool_reps,
                          "ark_bytes_compressed": os.path.getsize(os.path.join(dirs["compressed"], "feats.ark")),
                          "ark_bytes_uncompressed": os.path.getsize(os.path.join(dirs["uncompressed"], "feats.ark")),
                          "s_compressed": spread(wall["compressed"]), "s_uncompressed": spread(wall["uncompressed"]),
                          "compressed_over_uncompressed": mc / mu, "pools_bitwise_equal": same}), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pool-reps", type=int, default=5)
    ap.add_argument("--minutes", type=int, nargs="*", default=[1, 10, 60])
    ap.add_argument("--long-minutes", type=int, nargs="*", default=[60], help="also as one utterance of this many minutes")
    args = ap.parse_args()
    for minutes in args.minutes:
        bench(minutes, args.reps, args.pool_reps)
    for minutes in args.long_minutes:
        bench(minutes, args.reps, args.pool_reps, one_utterance=True)


if __name__ == "__main__":
    main()
