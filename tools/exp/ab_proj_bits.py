"""Bit identity of fhvae_proj_bf16 (csrc/proj.hip) between two BUILDS of libfhvae_hip.so (tools/exp/ab_lib.py's method): one child
process per build loads its library, runs the projection on seeded operands -- the three shapes of the c3 training step (M = T B =
40,960: the from-above term, the decoder head's forward and its dh) and the small ring cases of tests/test_proj_ring_gpu.py (M =
65 and 16,391, N = 4, 128, 160, 256, K / 64 = 1 .. 9, 16, 17, 33, with a bias) -- and writes every C to a file; the parent compares
the files of the two builds byte for byte.  The kernel has no atomics and a fixed accumulation order per element (k ascending), so
any difference means the order moved or a ring slot was read before it landed.

    python tools/exp/ab_proj_bits.py parent=path/to/libfhvae_hip.so pr=path2
"""
import filecmp, hashlib, os, shutil, subprocess, sys, tempfile
HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [(40960, 256, 1024), (40960, 160, 256), (40960, 256, 192)]
CASES += [(M, N, 64 * nk) for M in (65, 16391) for N in (4, 128, 160, 256) for nk in (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 33)]


def name(M, N, K):
    return "c_%d_%d_%d.bin" % (M, N, K)


def child(path, outdir):
    sys.path.insert(0, os.path.join(HERE, "..", "..", "pytorch-scalablefhvae_amd"))
    import torch
    import hip_binding as hb
    hb.load_library(path)
    for M, N, K in CASES:
        g = torch.Generator()
        g.manual_seed(M * 1000003 + N * 1009 + K)
        a = torch.randn(M, K + 8, generator=g).bfloat16().cuda()[:, :K]  # lda, ldb > K
        w = torch.randn(N, K + 16, generator=g).bfloat16().cuda()[:, :K]
        bias = torch.randn(N, generator=g).cuda() if M != 40960 else None
        c = hb.proj_bf16(a, w, bias)
        torch.cuda.synchronize()
        c.cpu().numpy().tofile(os.path.join(outdir, name(M, N, K)))


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()[:16]


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    elif len(sys.argv) != 3 or not all("=" in a for a in sys.argv[1:]):
        sys.exit(__doc__)
    else:
        builds = [a.split("=", 1) for a in sys.argv[1:]]
        tmp = tempfile.mkdtemp(prefix="proj_bits_")
        try:
            for nm, path in builds:
                os.makedirs(os.path.join(tmp, nm))
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(path), os.path.join(tmp, nm)],
                                   capture_output=True, text=True, timeout=600)
                if r.returncode != 0:  # nothing more on the GPU after a failure
                    sys.exit("%s: exit %d\n%s" % (nm, r.returncode, r.stderr[-2000:]))
            (n0, _), (n1, _) = builds
            print("# C of fhvae_proj_bf16, builds %s and %s, seeded operands, lda = K + 8, ldb = K + 16; sha256[:16] of each build's bytes" % (n0, n1))
            diff = 0
            for M, N, K in CASES:
                f0, f1 = (os.path.join(tmp, nm, name(M, N, K)) for nm in (n0, n1))
                same = filecmp.cmp(f0, f1, shallow=False)
                diff += not same
                print("M %5d N %3d K %4d  %9d bytes  %s %s  %s" % (M, N, K, os.path.getsize(f0), sha(f0), sha(f1), "identical" if same else "DIFFERENT"))
            print("# %d of %d cases differ" % (diff, len(CASES)))
            sys.exit(1 if diff else 0)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
