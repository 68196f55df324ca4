"""Distributed hierarchical sampling: two ranks sharing ONE MI355X (gloo staged through the host; the kernels, the row-sharded
K-row table, the block merge and both fused-Adam arenas are the product code) run one epoch of DistributedHierarchicalTrainer
and must reproduce a single-process HierarchicalTrainer fed the same global batches: the rows loaded at every block start,
every step's loss and the parameters at the end."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

K, BG, SEQS, NSEG, SEED = 7, 16, 21, 150, 3  # K odd: the last shard is ragged (rows [0, 4) and [4, 7)); 3 blocks per epoch
CFG = {"f32": dict(T=20, F=16, H=32, D=16), "bf16": dict(T=20, F=80, H=128, D=32)}


def _data(mode):
    c = CFG[mode]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(NSEG, c["T"], c["F"], generator=g)
    idx = torch.randint(0, SEQS, (NSEG,), generator=g)
    ns = torch.randint(20, 200, (NSEG,), generator=g)
    e2, e1 = torch.randn(NSEG, c["D"], generator=g), torch.randn(NSEG, c["D"], generator=g)  # one draw per pool segment
    return x, idx, ns, e2, e1


def _build(mode):
    from fhvae import FHVAE

    c = CFG[mode]
    torch.manual_seed(17)
    H = c["H"]
    return FHVAE(c["T"] * c["F"], [H, H], [H, H], c["D"], c["D"], [H, H], seg_len=c["T"], num_seqs=K, reference_compat=False,
                 compute_dtype=mode).cuda()


class _Recorder:
    """The pool, recording the segment ids of the last batch (the step's reparameterisation draws are looked up by them)."""

    def __init__(self, pool):
        self.pool, self.ids = pool, None
        self.seq_ptr, self.seq_counts, self.num_seqs = pool.seq_ptr, pool.seq_counts, pool.num_seqs

    def features(self, ids):
        return self.pool.features(ids)

    def batch(self, ids):
        self.ids = ids
        return self.pool.batch(ids)


def _setup(mode):
    from datasets import SyntheticSegmentPool

    x, idx, ns, e2, e1 = _data(mode)
    m = _build(mode)
    rec = _Recorder(SyntheticSegmentPool(x, idx, ns, SEQS, torch.device("cuda")))
    # eps by pool segment (SyntheticSegmentPool sorts the split by sequence: the same order here)
    order = torch.sort(idx, stable=True).indices
    e2, e1 = e2[order].cuda(), e1[order].cuda()
    fwd = m.forward
    m.forward = lambda *a, **k: fwd(*a, eps=(e2[rec.ids], e1[rec.ids]), **k)
    return m, rec


def _block_estimate(m, pool, seg_ids, local_idx, N, chunk):
    """The one-process estimate of a block from the current weights (HierarchicalTrainer.estimate + load's arithmetic)."""
    import hip_binding as hb
    from hierarchical import mu2_ratio

    est = hb.SortedMu2Estimator(K, m.z2_dim, seg_ids.device)
    with torch.no_grad():
        for c0 in range(0, N, chunk):
            c1 = min(N, c0 + chunk)
            est.add(m.encode_z2(pool.features(seg_ids[c0:c1])), local_idx[c0:c1])
    return est.result(mu2_ratio(m))[0]


def _worker(rank, world, port, mode, ret):
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "pytorch-scalablefhvae_amd")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if mode == "bf16":
        os.environ["FHVAE_NO_CLUSTER"] = "1"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dist_shard import DistributedFHVAE
    from hierarchical import DistributedHierarchicalTrainer

    m, rec = _setup(mode)
    runner = DistributedFHVAE(m, lr=1e-3, betas=(0.95, 0.999))
    losses = []

    def step(li, x, ns):
        out = runner.train_step(x, li, ns, alpha=10.0)
        losses.append(out[0].item())
        return out

    tr = DistributedHierarchicalTrainer(runner, rec, K, BG, step, seed=SEED, chunk=32, log=None)
    loads = []
    est, load = tr.estimate, tr.load
    seen = {}

    def estimate(N):
        seen["N"] = N
        est(N)

    def load_and_record():
        want = _block_estimate(m, rec, tr.seg_ids, tr.local_idx, seen["N"], 32)  # same weights, one process, whole block
        load()
        loads.append((runner.gather_table().cpu(), want.cpu()))

    tr.estimate, tr.load = estimate, load_and_record
    total, nb, nseg, rc = tr.run_epoch(0)
    full = runner.state_dict()
    ret[rank] = dict(losses=losses, loads=loads, nb=nb, rc=rc, rows=(runner.sh.row0, runner.sh.row1),
                     table=full["state_dict"]["mu2_table"].cpu(), status=runner.check_status(),
                     w=m.z2_pre_encoder.lstm.weight_hh_l1.detach().cpu(), wd=m.pre_decoder.lstm.weight_ih_l0.detach().cpu(),
                     wh=m.dec_gauss_layer.mulayer.weight.detach().cpu(), skipped=tr.skipped)
    dist.destroy_process_group()


def _single_process(mode, world):
    """HierarchicalTrainer (unchanged) on one process, its pass cut by the same tail rule so it sees the same global batches."""
    import hip_binding as hb
    from dist_shard import rank_slice
    from hierarchical import HierarchicalTrainer
    from hip_optim import FusedAdam
    from train_model import loss_function

    m, rec = _setup(mode)
    opt = FusedAdam(m.parameters(), lr=1e-3, betas=(0.95, 0.999))
    losses, loads = [], []

    def step(li, x, ns):
        opt.zero_grad()
        out = m(x, li, K, ns)
        loss = loss_function(out[0], out[1], 10.0)
        hb.backward(loss)
        opt.step()
        losses.append(loss.item())
        return loss.detach(), out[0].detach()

    class SameBatches(HierarchicalTrainer):
        def load(self):
            super().load()
            loads.append(m.mu2_table.detach().cpu().clone())

        def train_pass(self, N):
            perm = torch.randperm(N, device=self.dev, generator=self.gen)
            total, nb = torch.zeros((), device=self.dev), 0
            for s in range(0, N, self.B):
                sel = perm[s:s + self.B]
                _, b, _ = rank_slice(sel.shape[0], world, world - 1)  # keep the first n - n % W: what the ranks train together
                if b == 0:
                    continue
                ids = self.seg_ids[sel[:b]]
                _, x, ns = self.pool.batch(ids)
                total += self.step_fn(self.local_idx[sel[:b]], x, ns)[0]
                nb += 1
            return total, nb

    tr = SameBatches(m, opt, rec, K, BG, step, seed=SEED, chunk=32, log=None)
    tr.run_epoch(0)
    return m, losses, loads


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_two_ranks_hierarchical_match_single_process(mode):
    world = 2
    old = os.environ.get("FHVAE_NO_CLUSTER")
    if mode == "bf16":
        os.environ["FHVAE_NO_CLUSTER"] = "1"
    try:
        m, ref_losses, ref_loads = _single_process(mode, world)
        ret = mp.Manager().dict()
        mp.spawn(_worker, args=(world, 29300 + os.getpid() % 150 + (0 if mode == "f32" else 160), mode, ret), nprocs=world,
                 join=True)
    finally:
        if old is None:
            os.environ.pop("FHVAE_NO_CLUSTER", None)
        else:
            os.environ["FHVAE_NO_CLUSTER"] = old
    r0, r1 = ret[0], ret[1]
    assert r0["rows"] == (0, 4) and r1["rows"] == (4, 7)
    assert r0["status"] == 0 and r0["rc"] is None and r0["nb"] == r1["nb"] == len(ref_losses) >= 6
    assert len(r0["loads"]) == len(ref_loads) == 3  # three blocks
    for j, ((got, want), ref) in enumerate(zip(r0["loads"], ref_loads)):
        # the merged rows against the one-process estimate from the same weights (split ranges, rank-order sum): 1e-6 relative
        torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-6 * float(want.abs().max()), msg="block %d" % j)
        assert torch.equal(got, r1["loads"][j][0])  # identical on every rank
        if j == 0:  # the first block starts from the same weights as the single process: the same rows
            torch.testing.assert_close(got, ref, rtol=1e-6, atol=1e-6 * float(ref.abs().max()))
    tol_l, tol_p = (2e-4, dict(rtol=2e-4, atol=1e-4)) if mode == "f32" else (5e-4, dict(rtol=1e-3, atol=3e-4))
    for k, want in enumerate(ref_losses):  # the global loss = the mean of the two local losses (equal local batch sizes)
        got = 0.5 * (r0["losses"][k] + r1["losses"][k])
        assert abs(got - want) <= tol_l * abs(want), (k, got, want)
    for key, p in (("w", m.z2_pre_encoder.lstm.weight_hh_l1), ("wd", m.pre_decoder.lstm.weight_ih_l0),
                   ("wh", m.dec_gauss_layer.mulayer.weight)):
        torch.testing.assert_close(r0[key], p.detach().cpu(), **tol_p)
        assert torch.equal(r0[key], r1[key])  # replicas stay bit-identical
    torch.testing.assert_close(r0["table"], m.mu2_table.detach().cpu(), **tol_p)
