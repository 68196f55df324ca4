"""SHA-256 of what the all-pairs kernels (csrc/sv.hip, csrc/tsne.hip, the f32 K5 of csrc/disc_mfma.hip and the bf16 K5 of
csrc/disc_lp.hip) write, on seeded inputs -- one line "name digest" per output, for comparing two builds of the library bit for bit.

    python tools/allpairs_digest.py [--lib PATH/libfhvae_hip.so] > listing.txt
    python tools/allpairs_digest.py --compare PARENT_RUN1 PARENT_RUN2 RESULT

--compare: an output whose two parent digests differ is not reproducible and is listed as such; every other output must have
the parent's digest in RESULT (exit status 1 otherwise).  The digests pin compiler and library together: they are evidence
for one change on one toolchain, not a regression test.
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-scalablefhvae_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SV_EXTRA = [(130, 48, 1024, 6, 5), (130, 128, 1024, 6, 6)]  # (D = 48: 12 chunks per row under the 4-chunk swizzle)
TSNE_EXTRA = [(130, 48, 8.0)]
# (B, S, D, regime, pattern, lp); lp: the bf16 compute mode (its own kernel for D = 32)
K5 = [(257, 4097, 32, "unrelated", "edges", False), (300, 4633, 16, "separated", "edges", False), (2048, 33, 32, "unrelated", "edges", False),
      (257, 4097, 32, "unrelated", "edges", True), (300, 4633, 32, "separated", "edges", True), (2048, 33, 32, "unrelated", "edges", True)]


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def listing():
    import numpy as np
    import torch

    import disc_compare as DC
    import hip_binding as hb
    import sv_ref
    import test_sv_gpu
    import test_tsne_gpu
    import tsne_ref

    def dev(a):
        return torch.from_numpy(np.array(a)).cuda()

    for S, D, NB, speakers, seed in test_sv_gpu.CASES + SV_EXTRA:
        emb, label = sv_ref.make_case(S, D, speakers, seed)
        yield "sv S%d D%d NB%d hist" % (S, D, NB), hb.sv_hist(dev(emb), dev(label), NB)

    for seed, (N, D, perp) in enumerate(test_tsne_gpu.CASES + TSNE_EXTRA):
        what = "tsne N%d D%d p%g " % (N, D, perp)
        x = dev(tsne_ref.center(tsne_ref.make_case(N, D, 6, seed)[0]))
        beta, m, z = hb.tsne_affinity(x, perp)
        for name, t in (("beta", beta), ("m", m), ("z", z)):
            yield what + name, t
        y = dev(tsne_ref.y0(N, 0))
        out, scal = hb.tsne_grad(x, beta, m, z, y, 12.0)
        yield what + "grad out", out
        yield what + "grad scal", scal
        v, g, ws = torch.zeros_like(y), torch.ones_like(y), hb.tsne_workspace(x)
        for it in range(5):
            a, mom = tsne_ref.schedule(it)
            hb.tsne_step(x, beta, m, z, y, v, g, a, mom, tsne_ref.learning_rate(N), ws=ws)
        yield what + "Y after 5 steps", y

    gsc = torch.tensor([0.7], device="cuda")
    for seed, (B, S, D, regime, pattern, lp) in enumerate(K5):
        what = "k5 %s B%d S%d D%d " % ("bf16" if lp else "f32", B, S, D)
        q, t, idx = (a.cuda() for a in DC.make_inputs(B, S, D, regime, pattern, seed))
        rmax, rsum, tgt, ce = hb.raw_disc_fwd(q, t, idx, lp=lp)
        for name, r in (("rmax", rmax), ("rsum", rsum), ("tgt", tgt), ("ce", ce)):
            yield what + "fwd " + name, r
        for name, ws_bytes in (("one pass", None), ("two passes", 0)):
            sink = torch.zeros(S, D, device="cuda")
            dq, _ = hb.raw_disc_bwd(q, t, idx, rmax, rsum, gsc, 1.0 / B, dt_sink=sink, lp=lp, ws_bytes=ws_bytes)
            yield what + "bwd %s dq" % name, dq
            yield what + "bwd %s dt" % name, sink


def read(path):
    with open(path) as f:
        return dict(line.rstrip("\n").rsplit(" ", 1) for line in f if line.strip())


def compare(p1, p2, res):
    a, b, r = read(p1), read(p2), read(res)
    assert list(a) == list(b) == list(r), "the three listings name different outputs"
    skipped = [k for k in a if a[k] != b[k]]
    differ = [k for k in a if a[k] == b[k] and r[k] != a[k]]
    print("%d outputs; %d not reproducible by the parent itself (not compared); %d of the other %d differ" % (len(a), len(skipped), len(differ), len(a) - len(skipped)))
    print("%-44s %-16s %-16s %-16s" % ("output", "parent, run 1", "parent, run 2", "result"))
    for k in a:
        note = "   not reproducible" if k in skipped else "   DIFFERS" if k in differ else ""
        print("%-44s %-16s %-16s %-16s%s" % (k, a[k][:16], b[k][:16], r[k][:16], note))
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="the library to load (default: the tree's own, built if need be)")
    ap.add_argument("--compare", nargs=3, metavar="LISTING")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    import hip_binding as hb

    if args.lib:
        hb.load_library(args.lib)
    else:
        import build_ext

        build_ext.build(verbose=False)
    for name, t in listing():
        print(name, digest(t), flush=True)


if __name__ == "__main__":
    main()
