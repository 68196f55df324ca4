"""FLAC decoding on one MI355X (fhvae_flac_scan / fhvae_flac_decode, csrc/flac.hip) -- prints one JSON line per measurement,
for 1 min, 10 min and 1 h of 16 kHz mono 16-bit audio in 10 s utterances.  The audio is coded by the test-side encoder
(tests/flac_ref.py: LPC order 8 fitted per utterance, 4096-sample blocks, Rice partitions of 256) from --distinct different
utterances that are then repeated: what decoding costs does not depend on the files being different.

  kernels: HIP-event time of the scan, of the parse pass (every candidate to its end with its CRC-16, no output) and of the
           decode pass (the chain's frames into the output), each with its own pair of events, alternated with fhvae_feats_fwd
           on the same audio; medians with minimum and maximum.  And the host-to-device copy of the equivalent 16-bit PCM from
           pinned memory, which is what a corpus stored as WAV has to move instead.
  cli:     wall time of prepare_numpy_data.prepare_numpy over the longest corpus stored as FLAC and stored as WAV, alternated.

    python tools/bench_flac.py [--reps 10] [--cli-reps 3] [--minutes 1 10 60] [--distinct 4] [--skip-cli] [--out FILE]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import wave

import numpy as np

import bench_common  # (importing it sets the package's import path)

sys.path.insert(0, os.path.join(bench_common.ROOT, "tests"))

SR, UTT, BLOCK = 16000, 160000, 4096


def utterance(seed):
    """10 s of voiced-speech-like audio: a harmonic series with a moving pitch and envelope plus noise, int16."""
    rng = np.random.default_rng(seed)
    t = np.arange(UTT) / SR
    f0 = 110 + 40 * np.sin(2 * np.pi * (0.3 + 0.1 * seed) * t) + 20 * seed
    ph = 2 * np.pi * np.cumsum(f0) / SR
    y = sum(np.sin(k * ph) / k ** 1.5 for k in range(1, 12)) * (0.5 + 0.45 * np.sin(2 * np.pi * 2.5 * t)) + 0.02 * rng.standard_normal(UTT)
    return np.round(0.25 * y / np.abs(y).max() * 32767).astype(np.int64)


def encode(x):
    """The utterance as a FLAC file: LPC order 8 (least squares over the utterance, 12-bit coefficients, shift 10)."""
    import flac_ref as R

    order = 8
    A = np.stack([x[order - 1 - i:len(x) - 1 - i] for i in range(order)], axis=1).astype(np.float64)
    c = np.linalg.lstsq(A, x[order:].astype(np.float64), rcond=None)[0]
    coefs = np.clip(np.round(c * 1024), -2048, 2047).astype(int).tolist()
    n_full = len(x) // BLOCK
    return R.encode_stream(x[:, None], 16, SR, block=BLOCK,
                           subs=lambda fi, ch: R.Sub("lpc", coefs=coefs, precision=12, shift=10, part_order=4 if fi < n_full else 0))


def spread4(ts):
    return {k: round(v, 4) for k, v in bench_common.spread(ts).items()}


def timed(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def bench_kernels(minutes, blobs, pcm, reps):
    import torch

    import features as F
    import flac_lite
    import hip_binding as hb

    U = max(1, minutes * 6)
    files = [blobs[j % len(blobs)] for j in range(U)]
    infos = [flac_lite.parse_flac(b) for b in files]
    lens = [len(b) - i.first_frame for b, i in zip(files, infos)]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dev = torch.device("cuda")
    host = np.concatenate([np.frombuffer(b, np.uint8, offset=i.first_frame) for b, i in zip(files, infos)])
    buf = torch.from_numpy(host).to(dev)
    desc = np.zeros(U, hb.FLAC_DESC)
    desc["byte_begin"], desc["byte_end"], desc["rate"], desc["channels"], desc["bps"] = ptr[:-1], ptr[1:], SR, 1, 16
    desc["min_block"], desc["n_samples"], desc["out_off"] = BLOCK, UTT, np.arange(U) * UTT
    desc_d = torch.from_numpy(desc.view(np.uint8)).to(dev)
    info = torch.empty(buf.numel(), dtype=torch.int32, device=dev)
    hb.flac_scan(buf, desc_d, info)
    cand = torch.nonzero(info).flatten()
    nc = cand.numel()
    st, end, spos = (torch.empty(nc, dtype=dt, device=dev) for dt in (torch.int32, torch.int64, torch.int64))
    hb.flac_decode(buf, desc_d, cand, st, end, spos)
    # the chain: here simply the candidates that parse and whose end is a candidate or a file's end (checked against the PCM below)
    ok = (st == 0) & (torch.isin(end, cand) | torch.isin(end, torch.from_numpy(ptr[1:]).to(dev)))
    chain = cand[ok]
    out = torch.empty(U * UTT, dtype=torch.int32, device=dev)
    st2, end2, spos2 = (torch.empty(chain.numel(), dtype=dt, device=dev) for dt in (torch.int32, torch.int64, torch.int64))
    hb.flac_decode(buf, desc_d, chain, st2, end2, spos2, out)
    want = torch.from_numpy(np.concatenate([pcm[j % len(pcm)] for j in range(U)]).astype(np.int32)).to(dev)
    exact = bool(torch.equal(out, want)) and int(st2.abs().sum().item()) == 0

    n_fft, hop, n_mels = F.frame_sizes(SR) + (80,)
    wl = np.full(U, UTT, dtype=np.int64)
    frames = F.num_frames(wl, n_fft, hop)
    wave_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(wl)])).to(dev)
    frame_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(frames)])).to(dev)
    y = want.to(torch.float32) / 32768.0
    dft, mel = torch.from_numpy(F.dft_basis(n_fft)).to(dev), torch.from_numpy(F.mel_basis(SR, n_fft, n_mels)).to(dev)
    feats = torch.empty((int(frames.sum()), n_mels), device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    pinned = torch.from_numpy(np.concatenate([pcm[j % len(pcm)] for j in range(U)]).astype(np.int16)).pin_memory()
    pcm_d = torch.empty(U * UTT, dtype=torch.int16, device=dev)
    steps = {
        "scan": lambda: hb.flac_scan(buf, desc_d, info),
        "parse": lambda: hb.flac_decode(buf, desc_d, cand, st, end, spos),
        "decode": lambda: hb.flac_decode(buf, desc_d, chain, st2, end2, spos2, out),
        "feats_fwd": lambda: hb.feats_fwd(y, wave_ptr, frame_ptr, dft, mel, n_fft, hop, n_mels, "fbank", feats, status),
        "h2d_pcm16": lambda: pcm_d.copy_(pinned, non_blocking=True),
    }
    for fn in steps.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in steps}
    for _ in range(reps):
        for k, fn in steps.items():
            ts[k].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in ts.items()}
    return {"bench": "flac_kernels", "audio_min": minutes, "utterances": U, "flac_bytes": int(buf.numel()), "pcm16_bytes": 2 * U * UTT,
            "candidates": int(nc), "frames": int(chain.numel()), "reps": reps, "decoded_equals_pcm": exact,
            "ms": {k: spread4(v) for k, v in ts.items()},
            "flac_total_over_feats_fwd": round((med["scan"] + med["parse"] + med["decode"]) / med["feats_fwd"], 2)}


def bench_cli(minutes, blobs, pcm, reps, root):
    import prepare_numpy_data as P

    U = max(1, minutes * 6)
    for kind in ("flac", "wav"):
        d = os.path.join(root, kind, "train")
        os.makedirs(d)
        lines = []
        for j in range(U):
            p = os.path.join(d, "u%05d.%s" % (j, kind))
            if kind == "flac":
                with open(p, "wb") as fh:
                    fh.write(blobs[j % len(blobs)])
            else:
                with wave.open(p, "wb") as w:
                    w.setnchannels(1)
                    w.setsampwidth(2)
                    w.setframerate(SR)
                    w.writeframes(pcm[j % len(pcm)].astype("<i2").tobytes())
            lines.append("u%05d %s\n" % (j, p))
        with open(os.path.join(d, "wav.scp"), "w") as fh:
            fh.writelines(lines)
    wall = {"flac": [], "wav": []}
    split = {"flac": {}, "wav": {}}
    for r in range(reps + 1):  # (the first round warms up: files into the page cache, bases onto the device)
        for kind in wall:
            t = {}
            t0 = time.perf_counter()
            P.prepare_numpy("bench", "train", os.path.join(root, kind), os.path.join(root, kind + "_np"), "fbank", SR, timings=t)
            if r:
                wall[kind].append(time.perf_counter() - t0)
                split[kind] = {k: round(v, 3) for k, v in t.items()}
    a = np.load(os.path.join(root, "flac_np", "train", "u00000.npy"))
    b = np.load(os.path.join(root, "wav_np", "train", "u00000.npy"))
    return {"bench": "prepare_numpy_data_flac_vs_wav", "audio_min": minutes, "files": U, "reps": reps, "s_flac": spread4(wall["flac"]),
            "s_wav": spread4(wall["wav"]), "flac_over_wav": round(float(np.median(wall["flac"]) / np.median(wall["wav"])), 3),
            "last_split_flac": split["flac"], "last_split_wav": split["wav"], "features_bitwise_equal": bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--minutes", type=int, nargs="*", default=[1, 10, 60])
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import build_ext

    build_ext.build(verbose=False)
    t0 = time.time()
    pcm = [utterance(s) for s in range(args.distinct)]
    blobs = [encode(x) for x in pcm]
    rows = [{"bench": "flac_corpus", "distinct_utterances": args.distinct, "flac_bytes_over_pcm16_bytes": round(sum(map(len, blobs)) / (2.0 * UTT * len(pcm)), 3),
             "encode_s": round(time.time() - t0, 1)}]
    print(json.dumps(rows[0]), flush=True)
    for m in args.minutes:
        rows.append(bench_kernels(m, blobs, pcm, args.reps))
        print(json.dumps(rows[-1]), flush=True)
    if not args.skip_cli:
        tmp = tempfile.mkdtemp(prefix="bench_flac_")
        try:
            rows.append(bench_cli(max(args.minutes), blobs, pcm, args.cli_reps, tmp))
            print(json.dumps(rows[-1]), flush=True)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
