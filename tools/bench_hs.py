"""Hierarchical sampling against plain training at c3 net shapes (2x256 LSTM nets, z1 = z2 = 32, B = 2048, bf16), on a seeded
synthetic resident pool (frames in HBM, segments cut by fhvae_segment_gather, SEGS segments per sequence).

  plain      model with an S-row table; steps over random segments (K5 over S rows per step)
  hs K       model with a K-row table; HierarchicalTrainer blocks: select + estimate + load + one shuffled pass

Both run the step as train_model.py --hip-graph does (one captured step replayed; the short last batch of a block eagerly).
Reported per leg: segments/s over whole blocks (estimate included; plain: over STEPS steps), the select / estimate / load time
per block (device events), the training state (parameter, gradient and moment arenas: the table's rows and its moments) and
the peak working memory above everything resident (pool, every leg's model) during the measured stretch.  Legs alternate over REPS repetitions (ABAB...) after a
warm-up; the median is printed.  One JSON line per leg, then a table.

    python tools/bench_hs.py [--S 28000 1000000] [--K 2000 5000] [--reps 2] [--blocks 2] [--steps 30]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-scalablefhvae_amd"))

T, F, H, D, B = 20, 80, 256, 32, 2048
SEGS, SHIFT = 8, 8


class SynthResidentPool:
    """S sequences of SEGS segments each (seg_shift 8 over (SEGS-1)*8+20 frames), frames N(0,1) in HBM; the surface
    HierarchicalTrainer reads (seq_ptr, seq_counts, seg_seq, features, batch)."""

    def __init__(self, S, seed, device):
        import hip_binding as hb

        self.hb, self.num_seqs, self.T = hb, S, T
        fr = (SEGS - 1) * SHIFT + T
        g = torch.Generator(device=device)
        g.manual_seed(seed)
        self.pool = torch.randn(S * fr, F, device=device, generator=g)
        seq = torch.arange(S, device=device).repeat_interleave(SEGS)
        self.seg_seq = seq
        self.seg_start = seq * fr + torch.arange(SEGS, device=device).repeat(S) * SHIFT
        self.seg_nsegs = torch.full_like(seq, SEGS)
        self.seq_counts = np.full(S, SEGS, dtype=np.int64)
        self.seq_ptr = torch.arange(S + 1, device=device, dtype=torch.int64) * SEGS

    def __len__(self):
        return self.seg_seq.shape[0]

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.pool, self.seg_seq, self.seg_start, self.seg_nsegs, self.seq_ptr))

    def features(self, ids):
        return self.hb.segment_gather(self.pool, self.seg_start[ids], T, None, None)

    def batch(self, ids):
        return self.seg_seq[ids], self.features(ids), self.seg_nsegs[ids]


def make_step(hb, model, opt, num_seqs):
    """train_model.py's eager step and its --hip-graph replay (captured on the first full batch; state put back afterwards)."""
    from train_model import loss_function

    def train_step(idx, x, ns):
        opt.zero_grad()
        out = model(x, idx, num_seqs, ns)
        loss = loss_function(out[0], out[1], 10.0)
        hb.backward(loss)
        opt.step()
        return loss.detach(), out[0].detach()

    graph = {}

    def step(idx, x, ns):
        if x.shape[0] != B:
            return train_step(idx, x, ns)
        if not graph:
            st = (idx.clone(), x.clone(), ns.clone())
            keep = [t.clone() for t in (opt.p_arena.flat, opt.m, opt.v, opt._step_buf)]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    train_step(*st)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                outs = train_step(*st)
            for t, k in zip((opt.p_arena.flat, opt.m, opt.v, opt._step_buf), keep):
                t.copy_(k)
            graph.update(g=g, st=st, outs=outs)
        for d, s in zip(graph["st"], (idx, x, ns)):
            d.copy_(s)
        graph["g"].replay()
        return graph["outs"]
    return step


def build(num_seqs):
    from fhvae import FHVAE
    from hip_optim import FusedAdam

    torch.manual_seed(0)
    m = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, num_seqs=num_seqs, reference_compat=False,
              compute_dtype="bf16").cuda()
    return m, FusedAdam(m.parameters(), lr=1e-3, betas=(0.95, 0.999))


def state_mb(opt):
    """parameters, gradients and both Adam moments (the flat arenas): the table's part grows with its rows"""
    return 4 * opt.p_arena.flat.numel() * 4 / 2**20


class Plain:
    def __init__(self, hb, pool, steps):
        self.pool, self.steps = pool, steps
        self.model, self.opt = build(pool.num_seqs)
        self.step = make_step(hb, self.model, self.opt, pool.num_seqs)
        self.gen = torch.Generator(device="cuda")
        self.gen.manual_seed(1)

    def run(self, n_steps):
        for _ in range(n_steps):
            ids = torch.randint(0, len(self.pool), (B,), device="cuda", generator=self.gen)
            self.step(*self.pool.batch(ids))

    def measure(self):
        self.run(3)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.run(self.steps)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        return {"seg_per_s": self.steps * B / (ms / 1e3), "work_mb": (torch.cuda.max_memory_allocated() - base) / 2**20,
                "state_mb": state_mb(self.opt)}


class Hs:
    def __init__(self, hb, pool, K, blocks):
        from hierarchical import HierarchicalTrainer, plan_epoch

        self.model, self.opt = build(K)
        step = make_step(hb, self.model, self.opt, K)
        self.tr = HierarchicalTrainer(self.model, self.opt, pool, K, B, step, seed=0, log=None)
        self.plan = plan_epoch(self.tr.eligible, K, 0, 0)
        self.blocks, self.j = blocks, 0

    def next_block(self):
        blk = self.plan[self.j % len(self.plan)]
        self.j += 1
        return self.tr.run_block(blk)[2]

    def measure(self):
        self.next_block()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        nseg = 0
        e0.record()
        for _ in range(self.blocks):
            nseg += self.next_block()
            times.append(dict(self.tr.times))
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        per = {k: statistics.median(t[k] for t in times) for k in times[0]}
        return dict(per, seg_per_s=nseg / (ms / 1e3), segments_per_block=nseg / self.blocks,
                    work_mb=(torch.cuda.max_memory_allocated() - base) / 2**20, state_mb=state_mb(self.opt))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--S", type=int, nargs="+", default=[28000, 1000000])
    ap.add_argument("--K", type=int, nargs="+", default=[2000, 5000])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding as hb

    hb.load_library()
    hb.reset_device_words("cuda")
    rows = []
    for S in args.S:
        pool = SynthResidentPool(S, S, "cuda")
        legs = [("plain", lambda: Plain(hb, pool, args.steps))] + [("hs K=%d" % k, (lambda k=k: Hs(hb, pool, k, args.blocks)))
                                                                   for k in args.K]
        runners = {name: make() for name, make in legs}
        res = {name: [] for name, _ in legs}
        for r in range(args.reps):
            order = [n for n, _ in legs] if r % 2 == 0 else [n for n, _ in legs][::-1]
            for name in order:
                res[name].append(runners[name].measure())
        if hb.lstm_sync_status() != 0 or hb.diverged("cuda"):
            print("a persistent recurrence launch gave up or the loss diverged: results invalid", file=sys.stderr)
            return 3
        for name, _ in legs:
            rec = {k: statistics.median(x[k] for x in res[name]) for k in res[name][0]}
            rec.update(S=S, leg=name, reps=args.reps, pool_mb=pool.nbytes() / 2**20)
            print(json.dumps(rec))
            rows.append(rec)
        del runners
        del pool
        torch.cuda.empty_cache()
    print("%-9s %-9s %12s %10s %12s %9s %9s %9s %9s" % ("S", "leg", "segments/s", "select ms", "estimate ms", "load ms",
                                                        "state MB", "work MB", "pool MB"))
    for r in rows:
        print("%-9d %-9s %12.0f %10s %12s %9s %9.0f %9.0f %9.0f" % (
            r["S"], r["leg"], r["seg_per_s"], "%.3f" % r["select_ms"] if "select_ms" in r else "-",
            "%.2f" % r["estimate_ms"] if "estimate_ms" in r else "-", "%.3f" % r["load_ms"] if "load_ms" in r else "-",
            r["state_mb"], r["work_mb"], r["pool_mb"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
