"""Hierarchical sampling (Hsu & Glass, "Scalable Factorized Hierarchical Variational Autoencoder Training", Interspeech 2018):
training works through blocks of K sequences.  Before a block starts, the mu2 rows of its K sequences are set in closed form from
the current encoder (utils.py:45-60); the block's steps then use only those sequences' segments, and the discriminative loss runs
over only those K rows.  A step's cost and memory depend on K, not on the corpus size S.

  plan_epoch            host: the epoch's blocks (numpy Generator seeded from (seed, epoch)), every block K distinct sequences
  HierarchicalTrainer   device: per block select (fhvae_hs_select) -> estimate (encode_z2 + fhvae_mu2_accumulate_sorted)
                        -> load (the runner's load_block) -> one shuffled pass of training steps.  Written for W ranks; what
                        differs between one GPU and W ranks is behind the runner (hip_optim.LocalRunner: fhvae_mu2_load_table
                        into the FusedAdam arena; dist_shard.DistributedFHVAE: the row-sharded K-row table, the partials
                        all-gathered and summed in rank order by fhvae_mu2_merge_load_shard)
  DistributedHierarchicalTrainer  its constructor for a DistributedFHVAE
  estimate_pool_mu2     every sequence's mu2 of a pool by the same deterministic path (dev evaluation in this mode)

The model's table has K rows; row i holds the mu2 of the current block's i-th sequence, so a table row means nothing across blocks.
"""
from __future__ import annotations

import math
from typing import Callable, Optional

import numpy as np
import torch

from dist_shard import rank_range, rank_slice
from utils import mu2_ratio


def eligible_sequences(seq_counts) -> np.ndarray:
    """Sequences with at least one segment (the only ones a block may hold)."""
    return np.flatnonzero(np.asarray(seq_counts).reshape(-1) > 0).astype(np.int64)


def plan_epoch(eligible, K: int, seed: int, epoch: int) -> np.ndarray:
    """(ceil(S_elig / K), K) int64: the eligible sequences permuted by numpy.random.default_rng([seed, epoch]) and cut in order
    into blocks.  A short last block is topped up with sequences drawn without replacement from the rest of the permutation, so
    every block holds exactly K distinct sequences (the table shape and every captured-graph pointer stay fixed).  K must not
    exceed len(eligible) (clamp it first)."""
    eligible = np.asarray(eligible, dtype=np.int64)
    S = eligible.shape[0]
    if not 0 < K <= S:
        raise ValueError("K=%d must be in [1, %d] (the eligible sequences)" % (K, S))
    rng = np.random.default_rng([int(seed), int(epoch)])
    perm = rng.permutation(eligible)
    nb = math.ceil(S / K)
    short = nb * K - S
    if short:
        last0 = (nb - 1) * K
        extra = rng.choice(perm[:last0], size=short, replace=False)
        perm = np.concatenate([perm, extra])
    return perm.reshape(nb, K)


@torch.no_grad()
def estimate_pool_mu2(model, pool, chunk: int = 4096) -> torch.Tensor:
    """(pool.num_seqs, z2_dim) closed-form mu2 of every sequence of a pool grouped by sequence: encode_z2 over the segments in
    CSR order, in fixed chunks, summed by fhvae_mu2_accumulate_sorted (bitwise reproducible); rows of sequences without
    segments are 0.  One host sync (the status word)."""
    import hip_binding as hb

    dev = pool.seq_ptr.device
    est = hb.SortedMu2Estimator(pool.num_seqs, model.z2_dim, dev)
    ids = torch.arange(len(pool), device=dev)
    for c0 in range(0, len(pool), chunk):
        sel = ids[c0:c0 + chunk]
        est.add(model.encode_z2(pool.features(sel)), pool.seg_seq[sel])
    est.check()
    return est.result(mu2_ratio(model))[0]


class HierarchicalTrainer:
    """Runs the blocks of hierarchical sampling, on one GPU or on the W ranks of a distributed runner.

    model      FHVAE / SimpleFHVAE built with num_seqs=K (its mu2_table lives in `optimizer`'s arena)
    optimizer  hip_optim.FusedAdam over the model's parameters
    runner     the hip_optim.LocalRunner over both, when the caller has one (train_model); otherwise one is made here
    pool       datasets.ResidentSegmentPool or datasets.SyntheticSegmentPool (`seq_ptr`, `seq_counts`, `seg_seq`, `features`,
               `batch`)
    step_fn    step_fn(local_idx, features, nsegs) -> (loss, lower_bound): one training step with num_seqs = K (train_model's
               eager step or its --hip-graph replay)
    The shuffled pass of a block is torch.randperm(N, generator=self.gen), self.gen a CUDA generator seeded with `seed` once.
    The estimate runs encode_z2 over chunks of `chunk` segments in CSR order.

    On W ranks (DistributedHierarchicalTrainer: the K-row table row-sharded by dist_shard.DistributedFHVAE, rank r owns rows
    [row0, row1), the nets replicated):
    select     every rank selects the whole block (the plan and fhvae_hs_select are deterministic: identical on every rank)
    estimate   rank r encodes the contiguous range rank_range(N, W, r) of the block's CSR list into its own (K, D) sums; a
               sequence that crosses a range boundary is split over two ranks, which the merge makes whole
    merge      fhvae_hs_pack_partials -> ONE all-gather of (K, D+1) -> fhvae_mu2_merge_load_shard: the W partials of the own
               rows summed in rank order (independent of how the transport reduces: identical on every rank for a given W),
               loaded into the shard, its Adam moment rows zeroed
    train      the same seeded generator on every rank; each global batch of B is cut to a multiple of W (rank_slice) and rank
               r steps on its slice
    The status word is all-reduced (MAX) where it is read, so every rank raises together.
    """

    def __init__(self, model, optimizer, pool, K: int, batch_size: int, step_fn: Callable, seed: int = 0, chunk: int = 4096,
                 log: Optional[Callable] = print, runner=None):
        from fhvae_core import LocalTableOps
        from hip_optim import LocalRunner

        if not isinstance(model.table_ops, LocalTableOps):
            raise ValueError("HierarchicalTrainer needs the single-GPU mu2 table; a row-sharded table (dist_shard) is trained "
                             "by DistributedHierarchicalTrainer")
        if model.mu2_table is None or model.mu2_table.shape[0] != K:
            raise ValueError("hierarchical sampling with K=%d needs a model built with num_seqs=K" % K)
        runner = runner if runner is not None else LocalRunner(model, optimizer)
        self._setup(runner, pool, K, batch_size, step_fn, seed, chunk, log)

    def _setup(self, runner, pool, K, batch_size, step_fn, seed, chunk, log):
        import hip_binding as hb

        self.hb, self.runner, self.model, self.pool = hb, runner, runner.model, pool
        self.world, self.rank = runner.world, runner.rank
        self.K, self.B = int(K), int(batch_size)
        if self.B % self.world:
            raise ValueError("the batch size %d is not a multiple of the %d ranks" % (self.B, self.world))
        self.step_fn, self.chunk, self.log = step_fn, int(chunk), log
        self.seed = int(seed)
        self.eligible = eligible_sequences(pool.seq_counts)
        if self.K > len(self.eligible):
            raise ValueError("K=%d exceeds the %d sequences that have segments" % (self.K, len(self.eligible)))
        rows = runner.table_rows()[0]  # the table rows this rank owns (one GPU: all K)
        self.D, self.dev = int(rows.shape[1]), rows.device
        # capacity: the K longest sequences (no block can hold more segments)
        cap = int(np.sort(np.asarray(pool.seq_counts, dtype=np.int64))[::-1][:self.K].sum())
        self.seg_ids = torch.zeros(cap, dtype=torch.int64, device=self.dev)
        self.local_idx = torch.zeros(cap, dtype=torch.int64, device=self.dev)
        # words[0]: the block's segment count; low half of words[1]: the status word (one read gives both)
        self.words = torch.zeros(2, dtype=torch.int64, device=self.dev)
        self.n_out, self.status = self.words[0:1], self.words[1:2].view(torch.int32)[0:1]
        self.est = hb.SortedMu2Estimator(self.K, self.D, self.dev, status=self.status)
        # W ranks: this rank's partial sums and counts, packed for the one all-gather of the merge
        self.packed = torch.zeros(self.K, self.D + 1, device=self.dev, dtype=torch.float32) if self.world > 1 else None
        self.ratio = mu2_ratio(self.model)
        self.gen = torch.Generator(device=self.dev)
        self.gen.manual_seed(self.seed)
        self.times = {}  # the last block's select / estimate / load (W ranks: merge) times (ms, device events)
        self.skipped = 0  # segments of ragged last batches nobody trained (at most W - 1 per block; one GPU: none)

    def _read_words(self):
        if self.world > 1:
            # words[0] (the block's segment count) is the same on every rank; MAX over the status half raises on every rank at once
            self.runner.all_reduce_(self.words, op=torch.distributed.ReduceOp.MAX)
        h = self.words.cpu()
        st = int(h[1]) & 0xFFFFFFFF
        if st:
            raise RuntimeError("hierarchical sampling: %s (status %d)" % (self.hb.hs_status_message(st), st))
        return int(h[0])

    def select(self, block_seqs) -> int:
        """3a: the block's segments in CSR order into seg_ids / local_idx; returns their number (the one host sync per block)."""
        bs = torch.as_tensor(np.asarray(block_seqs, dtype=np.int64)).to(self.dev, non_blocking=False)
        if bs.shape != (self.K,):
            raise ValueError("a block holds exactly K=%d sequences" % self.K)
        self.hb.hs_select(self.pool.seq_ptr, bs, self.seg_ids, self.local_idx, self.n_out, self.status)
        return self._read_words()

    @torch.no_grad()
    def estimate(self, N: int):
        """3b: encode_z2 over this rank's range of the block's segments in fixed chunks, summed per local index without float
        atomics."""
        a, b = rank_range(N, self.world, self.rank)
        for c0 in range(a, b, self.chunk):
            c1 = min(b, c0 + self.chunk)
            z2 = self.model.encode_z2(self.pool.features(self.seg_ids[c0:c1]))
            self.est.add(z2, self.local_idx[c0:c1])

    def load(self):
        """3c: table rows = zsum / (count + r) in place in the arena, the table's m and v rows zeroed, accumulators cleared.
        FusedAdam keeps ONE step count, which keeps running: the fresh rows' first updates get the late-step bias correction
        of the nets (m and v warm up from 0 with factors ~1: steps of up to ~lr/sqrt(1-beta2) relative size on their first
        gradients, shrinking over ~1/(1-beta2) steps), as --continue-from from a reference checkpoint does (train_model.py)."""
        self.runner.load_block(self.est, self.packed, self.ratio)

    def train_pass(self, N: int):
        """3d: one device-side shuffled pass over the block's segments in batches of B, this rank's slice of each.  Returns
        (sum of losses (device), steps)."""
        perm = torch.randperm(N, device=self.dev, generator=self.gen)
        total = torch.zeros((), device=self.dev)
        nb = 0
        for s in range(0, N, self.B):
            sel = perm[s:s + self.B]
            a, b, skip = rank_slice(sel.shape[0], self.world, self.rank)
            self.skipped += skip
            if b == a:
                continue
            if self.world > 1:
                sel = sel[a:b]
            ids, li = self.seg_ids[sel], self.local_idx[sel]
            _, x, nsegs = self.pool.batch(ids)
            loss, _ = self.step_fn(li, x, nsegs)
            total += loss
            nb += 1
        return total, nb

    def run_block(self, block_seqs, j: int = 0, n_blocks: int = 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        skipped0 = self.skipped
        ev[0].record()
        N = self.select(block_seqs)
        ev[1].record()
        self.estimate(N)
        ev[2].record()
        self.load()
        ev[3].record()
        total, nb = self.train_pass(N)
        ev[3].synchronize()  # (the estimate and load only: the block's steps are queued behind them)
        skip, label = self.skipped - skipped0, self.runner.load_label
        self.times = {"select_ms": ev[0].elapsed_time(ev[1]), "estimate_ms": ev[1].elapsed_time(ev[2]),
                      label + "_ms": ev[2].elapsed_time(ev[3])}
        est_ms, load_ms = self.times["estimate_ms"], self.times[label + "_ms"]
        if self.log is not None and not self.runner.split_times:
            self.log("hs block %d/%d: %d seqs, %d segments, estimate %.2f ms" % (j + 1, n_blocks, self.K, N, est_ms + load_ms))
        elif self.log is not None:
            self.log("hs block %d/%d: %d seqs, %d segments, estimate %.2f ms, %s %.2f ms%s" % (
                j + 1, n_blocks, self.K, N, est_ms, label, load_ms,
                (", %d segments of the last batch skipped (not a multiple of %d ranks)" % (skip, self.world)) if skip else ""))
        return total, nb, N - skip

    def run_epoch(self, epoch: int, check: Optional[Callable] = None):
        """Every block of the epoch's plan.  `check(steps so far)` (optional) runs after each block and may return an exit code
        to stop.
        Returns (sum of losses (device), steps, segments, exit code or None)."""
        plan = plan_epoch(self.eligible, self.K, self.seed, epoch)
        total = torch.zeros((), device=self.dev)
        nb = nseg = 0
        for j, block in enumerate(plan):
            t, n, N = self.run_block(block, j, len(plan))
            total += t
            nb += n
            nseg += N
            if check is not None:
                rc = check(nb)
                if rc is not None:
                    return total, nb, nseg, rc
        self._read_words()  # the last block's estimate status
        return total, nb, nseg, None


class DistributedHierarchicalTrainer(HierarchicalTrainer):
    """HierarchicalTrainer over a dist_shard.DistributedFHVAE (its class docstring: what each step does on W ranks)."""

    def __init__(self, runner, pool, K: int, batch_size: int, step_fn: Callable, seed: int = 0, chunk: int = 4096,
                 log: Optional[Callable] = print):
        if runner.sh.S != K:
            raise ValueError("hierarchical sampling with K=%d needs a model built with num_seqs=K (the runner's table has %d rows)"
                             % (K, runner.sh.S))
        self._setup(runner, pool, K, batch_size, step_fn, seed, chunk, log)


def hs_clamp(K: int, seq_counts, log: Optional[Callable] = print) -> int:
    """K = min(K, sequences with at least one segment), with a line when it is clamped."""
    n = len(eligible_sequences(seq_counts))
    if n == 0:
        raise ValueError("hierarchical sampling: no sequence has a segment")
    if K > n:
        if log is not None:
            log("hs: --num-hierarchical-sequences %d clamped to %d (sequences with at least one segment)" % (K, n))
        return n
    if K <= 0:
        raise ValueError("--num-hierarchical-sequences must be positive")
    return int(K)
