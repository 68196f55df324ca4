"""tools/bench_infer.py -- reconstruct() of the c3 model (2 x 256 LSTM nets, z = 32, T = 20, F = 80) with the inference forward
(hip_binding.lstm_seq_infer) against the saving training forward (FHVAE_NO_INFER=1), alternated in one process.

    python tools/bench_infer.py [--calls 20] [--warmup 3] [--rounds 3]

One JSON line per case (bf16 at B = 2048 and 16384, f32 at B = 2048): segments/s from device events over --calls timed calls per
round (the best and the median round of each path), the peak allocated bytes of one call, and the gates / c bytes per net
the inference path does not write (from the shapes)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-scalablefhvae_amd")]

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="bf16:2048,bf16:16384,f32:2048")
    args = ap.parse_args()
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding as hb
    from fhvae import FHVAE

    T, F, H, L, D = 20, 80, 256, 2, 32
    for case in args.cases.split(","):
        dt, B = case.split(":")
        B = int(B)
        torch.manual_seed(0)
        m = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, num_seqs=1000, compute_dtype=dt).cuda()
        x = torch.randn(B, T, F, device="cuda")
        es = 2 if dt == "bf16" else 4
        res = {"case": "reconstruct c3 %s B=%d" % (dt, B), "gates_bytes_per_net": L * T * B * 4 * H * es,
               "c_bytes_per_net": L * T * B * H * 4}
        rates = {"infer": [], "no_infer": []}
        peaks = {}

        def run(path):
            if path == "no_infer":
                os.environ["FHVAE_NO_INFER"] = "1"
            else:
                os.environ.pop("FHVAE_NO_INFER", None)
            for _ in range(args.warmup):
                m.reconstruct(x)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                m.reconstruct(x)
            e1.record()
            torch.cuda.synchronize()
            peaks[path] = torch.cuda.max_memory_allocated() - base
            rates[path].append(B * args.calls / (e0.elapsed_time(e1) / 1e3))

        for _ in range(args.rounds):  # A/B alternated
            run("infer")
            run("no_infer")
        os.environ.pop("FHVAE_NO_INFER", None)
        for p in rates:
            res[p + "_segments_per_s_best"] = round(max(rates[p]))
            res[p + "_segments_per_s_median"] = round(statistics.median(rates[p]))
            res[p + "_peak_bytes"] = peaks[p]
        res["speedup_median"] = round(res["infer_segments_per_s_median"] / res["no_infer_segments_per_s_median"], 4)
        res["lstm_status"] = hb.lstm_sync_status()
        print(json.dumps(res), flush=True)
        del m, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
