"""Same-box A/B of two or more BUILDS of libfhvae_hip.so (tools/exp/ab_bwd.py's method for a change that is no run-time switch):
one child process per build and round, alternating, three rounds; a child loads its library, runs the c3 recurrence shapes (B =
2048, T = 20, H = 256, L = 2) and prints the us per forward call and per backward call (100 calls each after 5 warm-up calls).

    python tools/exp/ab_lib.py name=path/to/libfhvae_hip.so name2=path2 ...
"""
import os, subprocess, sys
HERE = os.path.dirname(os.path.abspath(__file__))


def child(path):
    sys.path.insert(0, os.path.join(HERE, "..", "..", "pytorch-scalablefhvae_amd"))
    import torch
    import hip_binding as hb
    hb.load_library(path)
    B, T, H, L = 2048, 20, 256, 2
    out = []
    for I, Ic in ((80, 0), (0, 64)):
        torch.manual_seed(0)
        lstm = torch.nn.LSTM(I + Ic, H, L)
        names = [n + "_l%d" % l for l in range(L) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        params = [getattr(lstm, n).detach().cuda().requires_grad_(True) for n in names]
        x = torch.randn(T, B, I).cuda() if I else None
        xc = torch.randn(B, Ic).cuda().requires_grad_(True) if Ic else None

        def timed(fn):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(100):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1000 / 100

        with torch.no_grad():
            fwd = timed(lambda: hb.lstm_seq(x, xc, T, params, hb.BF16))
        hs, hn = hb.lstm_seq(x, xc, T, params, hb.BF16)
        g = torch.randn_like(hs)
        bwd = timed(lambda: hs.backward(g, retain_graph=True))
        out.append("I=%d Ic=%d fwd %.1f bwd %.1f" % (I, Ic, fwd, bwd))
    assert hb.lstm_sync_status() == 0
    print(" | ".join(out), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    elif len(sys.argv) < 2 or not all("=" in a for a in sys.argv[1:]):
        sys.exit(__doc__)
    else:
        builds = [a.split("=", 1) for a in sys.argv[1:]]
        width = max(len(name) for name, _ in builds)
        print("us per call, B=2048 T=20 H=256 L=2 bf16 (fwd: one recurrence launch + casts; bwd: 2 recurrences + projection + weight gradients)")
        for rnd in range(3):
            for name, path in builds:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(path)], capture_output=True, text=True, timeout=120)
                if r.returncode != 0:  # nothing more on the GPU after a failure
                    sys.exit("round %d %s: exit %d\n%s" % (rnd, name, r.returncode, r.stderr[-2000:]))
                print("round %d %-*s %s" % (rnd, width, name, r.stdout.strip()), flush=True)
