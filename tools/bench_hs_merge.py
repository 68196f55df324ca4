"""Device time of the block merge of distributed hierarchical sampling on one GPU: fhvae_hs_pack_partials over a (K, D) estimate
and fhvae_mu2_merge_load_shard over W ranks' partials for one rank's rows (ceil(K / W) of them).  The all-gather between the two
moves W*K*(D+1)*4 bytes and is not measured here (one GPU has no peers).

    python tools/bench_hs_merge.py [--K 5000] [--D 32] [--W 8] [--reps 200]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-scalablefhvae_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=5000)
    ap.add_argument("--D", type=int, default=32)
    ap.add_argument("--W", type=int, default=8)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    import hip_binding as hb

    hb.load_library()
    dev = torch.device("cuda")
    K, D, W = a.K, a.D, a.W
    zsum, cnt = torch.randn(K, D, device=dev), torch.randint(0, 9, (K,), device=dev).float()
    packed = torch.empty(K, D + 1, device=dev)
    parts = torch.randn(W, K, D + 1, device=dev).abs()
    per = (K + W - 1) // W
    shard, m, v = (torch.empty(per, D, device=dev) for _ in range(3))

    def timed(fn):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps * 1e3

    pack_us = timed(lambda: hb.hs_pack_partials(zsum, cnt, packed))
    merge_us = timed(lambda: hb.mu2_merge_load_shard(parts, 0, per, shard, m, v, 0.25))
    print(json.dumps({"K": K, "D": D, "W": W, "pack_us": round(pack_us, 2), "merge_load_us": round(merge_us, 2),
                      "all_gather_bytes": W * K * (D + 1) * 4}))


if __name__ == "__main__":
    main()
