"""train_model.py -- the reference's training loop shape (train_model.py:243-261, :438-541) on the HIP
hot path.  Importing this module has no side effects (the reference parses argv at import time,
train_model.py:25-238, which makes `loss_function` un-importable; the CLI lives in `main()` here).

Kept from the reference: flag names and defaults of the flags the hot path reads (SURVEY section 2
row 5), `loss_function`, `check_terminate`, `check_best`, the per-batch order zero_grad -> forward ->
loss -> backward -> step, the NaN abort with exit code 2 (train_model.py:464-466), Adam with
betas (0.95, 0.999).  Not reproduced: the reference's defects listed in SURVEY 3.1 (fp64 cast,
wrong validation loss, double division, ...).  Data: synthetic (B,T,F) segments by default; real
feature scp files are SURVEY 8f "next" #1.
"""
from __future__ import annotations

import argparse
import functools
import os
import sys
import time
from typing import Optional

import numpy as np
import torch

from utils import check_best  # noqa: F401  (one body, in utils as in the reference; kept under this module's name)


# alpha/discriminative weight of 10 was found to produce best results (train_model.py:240)
def loss_function(lower_bound, log_qy, alpha=10.0):
    """Discriminative segment variational lower bound: -mean(lower_bound + alpha*log_qy)
    (train_model.py:243-251)."""
    if (isinstance(lower_bound, torch.Tensor) and isinstance(log_qy, torch.Tensor) and lower_bound.is_cuda and log_qy.is_cuda
            and lower_bound.dim() == 1 and log_qy.dim() == 0 and lower_bound.dtype == torch.float32 and log_qy.dtype == torch.float32):
        import hip_binding as hb  # the model's own outputs on the GPU: the same expression in one launch each way

        return hb.fused_loss(lower_bound, log_qy, alpha)
    return -1 * torch.mean(lower_bound + alpha * log_qy)


def check_terminate(epoch, best_epoch, patience, epochs):
    """train_model.py:254-261."""
    if (epoch - 1) - best_epoch > patience:
        return True
    if epoch > epochs:
        return True
    return False


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="ScalableFHVAE training on MI355X (HIP hot path)")
    p.add_argument("--model-type", default="fhvae", choices=["fhvae", "simple_fhvae"])  # train_model.py:140-144
    p.add_argument("--alpha-dis", type=float, default=10.0)                              # :48-53
    p.add_argument("--z1-hus", nargs=2, default=[128, 128])                               # :145-150 (strings from CLI)
    p.add_argument("--z2-hus", nargs=2, default=[128, 128])
    p.add_argument("--z1-dim", type=int, default=16)
    p.add_argument("--z2-dim", type=int, default=16)
    p.add_argument("--x-hus", nargs=2, default=[128, 128])
    p.add_argument("--seg-len", type=int, default=20)                                     # :120-123
    p.add_argument("--mels", type=int, default=80)
    p.add_argument("--training-batch-size", type=int, default=256)                        # :134-137
    p.add_argument("--dev-batch-size", type=int, default=2048)
    p.add_argument("--learning-rate", type=float, default=1e-3)
    p.add_argument("--beta-one", type=float, default=0.95)
    p.add_argument("--beta-two", type=float, default=0.999)
    p.add_argument("--epochs", type=int, default=100)
    p.add_argument("--patience", type=int, default=10)
    p.add_argument("--device", default="gpu")
    # synthetic-data controls (no reference counterpart: the reference reads scp files)
    p.add_argument("--num-seqs", type=int, default=100)
    p.add_argument("--train-segments", type=int, default=1000)
    p.add_argument("--dev-segments", type=int, default=250)
    p.add_argument("--seed", type=int, default=0)
    # real features in the reference's on-disk format (feats.scp / len.scp of .npy files, prepare_numpy_data.py:115-119)
    p.add_argument("--data-format", default="numpy", choices=["numpy", "kaldi"],              # train_model.py:38-43
                   help="what the feat-scp files point at: .npy files (prepare_numpy_data.py) or Kaldi archives "
                        "(prepare_kaldi_data.py, or any Kaldi recipe's feats.scp, compressed or not)")
    p.add_argument("--train-feat-scp", default=None)
    p.add_argument("--train-len-scp", default=None)
    p.add_argument("--dev-feat-scp", default=None)
    p.add_argument("--dev-len-scp", default=None)
    p.add_argument("--min-len", type=int, default=None)            # train_model.py:106-112 (defaults to seg_len, :267-268)
    p.add_argument("--mvn-path", default=None)                     # :113-119
    p.add_argument("--seg-shift", type=int, default=8)             # :124-126
    p.add_argument("--rand-seg", action="store_true")
    p.add_argument("--exp-dir", default=None, help="write the reference-layout checkpoint there after every epoch")
    p.add_argument("--hierarchical", dest="sample_hierarchical", action="store_true",   # train_model.py:203-214
                   help="re-estimate the mu2 table in closed form from the encoder before training (utils.py:45-60)")
    p.add_argument("--num-hierarchical-sequences", type=int, default=None,                 # train_model.py:203-214
                   help="hierarchical sampling (Hsu & Glass 2018): train through blocks of K sequences; before each block the "
                        "mu2 rows of its K sequences are set in closed form from the encoder, and the steps and the "
                        "discriminative loss use only those K rows (the model's table has K rows).  Off when not given")
    p.add_argument("--compute-dtype", default="f32", choices=["f32", "bf16"])
    p.add_argument("--hip-graph", action="store_true",
                   help="capture one training step (zero_grad, forward, loss, backward, Adam) into a hipGraph and replay it for "
                        "every full-size batch (static input buffers; a smaller last batch runs eagerly)")
    p.add_argument("--reference-objective", action="store_true",
                   help="train the reference's LITERAL objective: decoder outputs and mu2 detached inside the bound "
                        "(simple_fhvae.py:107,114) and log_qy = +CE (:122).  With a persistent learnable mu2 table that "
                        "objective pushes CE up without bound and gives the decoder no gradient; the default is the intended "
                        "objective (decoder trained, log_qy = -CE), which is also what bench.py and the README figures use")
    p.add_argument("--paper-objective", action="store_true", help="(accepted for compatibility: this is the default now)")
    p.add_argument("--continue-from", default=None,                 # train_model.py:192-197
                   help="checkpoint file (utils.save_checkpoint layout) to resume from: model, mu2 table, Adam moments and step")
    p.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                   help="process-group backend of the distributed mode (on when torchrun sets WORLD_SIZE > 1): nccl = RCCL, "
                        "the product transport; gloo stages device tensors through the host (tests: several ranks on one GPU)")
    p.add_argument("--check-interval", type=int, default=100,
                   help="batches between reads of the device-side divergence / recurrence-status words (each read is a host "
                        "sync; they are always read at the end of an epoch and before a checkpoint)")
    return p


def synthetic_split(n, T, F, S, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, T, F, generator=g)
    idx = torch.randint(0, S, (n,), generator=g)
    nsegs = torch.randint(20, 200, (n,), generator=g)
    return x, idx, nsegs


def dist_arg_error(args, world: int) -> Optional[str]:
    """Why the arguments cannot run on `world` ranks (None: they can)."""
    if args.training_batch_size % world:
        return ("--training-batch-size %d is not a multiple of the %d ranks: every global batch is cut into %d equal slices "
                "(the runner's 1/W gradient scale and its all-gather need equal local batches)" % (args.training_batch_size, world, world))
    if args.hip_graph and args.dist_backend != "nccl":
        return ("--hip-graph in distributed mode needs --dist-backend nccl: the captured step holds the runner's collectives, "
                "and gloo's (staged through the host) cannot be captured")
    return None


def _quiet(*_a, **_k):
    pass


def main(argv=None) -> int:
    """One process per GPU under torchrun when WORLD_SIZE > 1 (the distributed mode: dist_shard.DistributedFHVAE, the row-sharded
    table, rank 0 prints and writes); otherwise the single-GPU loop on cuda:0."""
    args = build_parser().parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        err = dist_arg_error(args, world)
        if err is not None:
            print(err, file=sys.stderr)
            return 1
    if args.device != "gpu" or not torch.cuda.is_available():
        print("this training path runs on a MI355X only (no CPU fallback)", file=sys.stderr)
        return 1
    if world <= 1:
        return _train(args, torch.device("cuda:0"), 1, 0)
    import torch.distributed as dist

    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    own = not dist.is_initialized()
    if own:
        dist.init_process_group(args.dist_backend, **({"device_id": device} if args.dist_backend == "nccl" else {}))
    try:
        return _train(args, device, dist.get_world_size(), dist.get_rank())
    finally:
        if own:
            dist.destroy_process_group()


class _Data:
    """The train and dev segments of a run: resident pools of real features (--train-feat-scp) or the synthetic splits.  The
    real / synthetic fork is decided here; the loop asks this object."""

    def __init__(self, args, device, world: int, rank: int):
        self.args, self.device, self.world, self.rank = args, device, world, rank
        self.real = args.train_feat_scp is not None
        T = args.seg_len
        if self.real:
            from datasets import KaldiDataset, NumpyDataset, ResidentSegmentPool

            Dataset = NumpyDataset if args.data_format == "numpy" else KaldiDataset  # train_model.py:371-374
            min_len = args.min_len if args.min_len is not None else T  # train_model.py:267-268
            tr_ds = Dataset(args.train_feat_scp, args.train_len_scp, min_len, args.mvn_path, T, args.seg_shift, args.rand_seg)
            dv_ds = Dataset(args.dev_feat_scp or args.train_feat_scp, args.dev_len_scp or args.train_len_scp, min_len,
                            args.mvn_path, T, args.seg_shift, False)
            self.tr_pool, self.dv_pool = ResidentSegmentPool(tr_ds, device), ResidentSegmentPool(dv_ds, device)
            self.F = self.tr_pool.pool.shape[1]
            self.S = len(tr_ds)  # len(train_loader.dataset), train_model.py:448
            self.n_train = len(self.tr_pool)
        else:
            self.F, self.S, self.n_train = args.mels, args.num_seqs, args.train_segments
        self.train = self.dev = None  # the synthetic splits (draw())
        self.counts = {"skipped": 0, "trained": 0}  # per epoch: segments of ragged last batches nobody trained, segments trained
        if world > 1:
            # every rank draws the same permutation (a generator of its own, seeded with --seed) and steps on its slice of each
            # global batch; only that slice's features are gathered
            self.order_dev = device if self.real else torch.device("cpu")
            self.perm_gen = torch.Generator(device=self.order_dev)
            self.perm_gen.manual_seed(args.seed)

    def draw(self, dev: bool = True):
        """The synthetic splits (x on the device, idx, nsegs) that are not drawn yet.  Hierarchical mode draws the train split
        before the model is built (K is clamped by its sequence counts); otherwise both are drawn after it."""
        if not self.real and self.train is None:
            self.train = self._split(self.args.train_segments, self.args.seed + 1)
        if not self.real and dev and self.dev is None:
            self.dev = self._split(self.args.dev_segments, self.args.seed + 2)

    def _split(self, n, seed):
        x, idx, nsegs = synthetic_split(n, self.args.seg_len, self.F, self.S, seed)
        return x.to(self.device), idx, nsegs

    def seq_counts(self):
        self.draw(dev=False)
        return self.tr_pool.seq_counts if self.real else np.bincount(self.train[1].numpy(), minlength=self.S)

    @functools.cached_property
    def hs_pools(self):
        """(train, dev) as pools grouped by sequence: what the hierarchical trainer and its dev estimate read."""
        if self.real:
            return self.tr_pool, self.dv_pool
        from datasets import SyntheticSegmentPool

        return tuple(SyntheticSegmentPool(x, idx, nsegs, self.S, self.device) for x, idx, nsegs in (self.train, self.dev))

    def _take(self, sel):
        x, idx, nsegs = self.train
        return idx[sel], x[sel], nsegs[sel]

    def train_batches(self, whole: bool = False):
        """One epoch of (idxs, features, nsegs).  One process (or `whole`: every rank sees all of it): real data by the pool's
        own shuffle, synthetic data by torch.randperm on the global CPU generator.  W ranks: this rank's slice of each batch."""
        B, (world, rank) = self.args.training_batch_size, ((1, 0) if whole else (self.world, self.rank))
        if self.real and world == 1:
            return self.tr_pool.epoch(B, shuffle=True)
        order = torch.randperm if world == 1 else (lambda n: torch.randperm(n, device=self.order_dev, generator=self.perm_gen))
        return _epoch_batches(self.n_train, B, world, rank, order, self.tr_pool.batch if self.real else self._take, self.counts)

    def dev_batches(self):
        B = self.args.dev_batch_size
        if self.real:
            return self.dv_pool.epoch(B, shuffle=False)
        x, idx, nsegs = self.dev
        return ((idx[s0:s0 + B], x[s0:s0 + B], nsegs[s0:s0 + B]) for s0 in range(0, x.shape[0], B))


def _epoch_batches(n: int, batch_size: int, world: int, rank: int, order, take, counts):
    """The train batches of one epoch on rank `rank` of `world`: `order(n)` is the epoch's permutation (the same on every rank),
    cut into global batches of `batch_size`; each is cut down to a multiple of `world` (rank_slice: one process skips nothing)
    and `take(positions)` gathers this rank's slice.  `counts`: the segments nobody ("skipped") / the ranks together trained."""
    from dist_shard import rank_slice

    perm = order(n)
    for s0 in range(0, n, batch_size):
        sel = perm[s0:s0 + batch_size]
        a, b, skip = rank_slice(sel.shape[0], world, rank)
        counts["skipped"] += skip
        counts["trained"] += (b - a) * world
        if b > a:
            yield take(sel[a:b] if world > 1 else sel)


def _build_model(args, input_size, num_seqs, say):
    from fhvae import FHVAE
    from simple_fhvae import SimpleFHVAE

    kw = dict(num_seqs=num_seqs, reference_compat=bool(args.reference_objective))
    if args.reference_objective:
        say("WARNING: --reference-objective trains the reference's literal loss (+CE, detached decoder); "
            "throughput/ELBO figures of this build use the default objective", file=sys.stderr)
    if args.model_type == "fhvae":
        return FHVAE(input_size, args.z1_hus, args.z2_hus, args.z1_dim, args.z2_dim, args.x_hus, seg_len=args.seg_len,
                     compute_dtype=args.compute_dtype, **kw)
    return SimpleFHVAE(input_size, args.z1_hus, args.z2_hus, args.z1_dim, args.z2_dim, args.x_hus, **kw)


def _resume(args, model, runner, num_rows, hs_K, input_size, say):
    """--continue-from: the checkpoint into the live model and optimizers -> (start_epoch, best_epoch, best_val_lb)."""
    ck = torch.load(args.continue_from, map_location="cpu", weights_only=False)
    start_epoch = int(ck["epoch"]) + 1  # saved at the end of an epoch
    best_val_lb = float(ck["best_val_lb"]) if ck.get("best_val_lb") is not None else -np.inf
    best_epoch = int(ck.get("best_epoch", start_epoch - 1))  # the patience window continues where it stood
    if runner.world > 1:
        # a checkpoint of this build (one GPU or distributed: the same layout) -> every rank keeps its own rows
        ck_table = ck["state_dict"].get("mu2_table")
        if ck_table is None or ck_table.shape[0] != num_rows:
            raise ValueError("--continue-from in distributed mode needs a checkpoint of this build with a %d-row mu2 table; it has %s"
                             % (num_rows, tuple(ck_table.shape) if ck_table is not None else "none"))
        runner.load_state_dict(ck)
    else:
        # resume (train_model.py:303-322 -> utils.load_checkpoint_file): weights + table into the live model, Adam moments and
        # step count into the arenas; the reference's own branch never rebuilds the optimizer (dead path)
        from utils import load_checkpoint

        ck_model, _values, optim_state, _, _, _ = load_checkpoint(ck, False, input_size=input_size)
        ck_sd = ck_model.state_dict()
        if hs_K is not None and ("mu2_table" not in ck_sd or ck_sd["mu2_table"].shape[0] != hs_K):
            raise ValueError("--continue-from with --num-hierarchical-sequences %d needs a checkpoint with a %d-row mu2 table "
                             "(a hierarchical checkpoint of the same K); it has %s" % (
                                 hs_K, hs_K, tuple(ck_sd["mu2_table"].shape) if "mu2_table" in ck_sd else "none"))
        ref_layout = "mu2_table" not in ck_sd  # a checkpoint of the reference itself: it never kept a table (simple_fhvae.py:51)
        model.load_state_dict(ck_sd, strict=not ref_layout)
        if optim_state is not None:
            if ref_layout:
                optim_state = _shift_reference_moments(optim_state, model, ck_model)
            runner.optimizer.load_state_dict(optim_state)
    say(f"resumed from {args.continue_from}: starting at epoch {start_epoch}")
    return start_epoch, best_epoch, best_val_lb


def _shift_reference_moments(optim_state, model, ck_model):
    """torch.optim.Adam's state over the reference's parameters (the nets, in named_parameters() order): ours has the table in
    front -> shift by one.  The table's moments start at zero while FusedAdam's ONE step counter continues from the checkpoint:
    the table's first updates therefore run without bias correction (m and v warm up from 0 with the nets' late-step factors
    ~1: steps of up to ~lr/sqrt(1-beta2) relative size on its first gradients, shrinking over ~1/(1-beta2) steps).  Harmless
    for a table the reference re-drew from N(0,1) on every forward (simple_fhvae.py:51), and stated here rather than hidden."""
    n_have = len(optim_state["param_groups"][0]["params"])
    net_params = [(n, p) for n, p in model.named_parameters() if p.requires_grad and n != "mu2_table"]
    n_nets = len(net_params)
    if n_have != n_nets:
        raise ValueError("--continue-from: the checkpoint's optimizer holds %d parameters, this model's nets have %d"
                         % (n_have, n_nets))
    # ... and the SAME parameters in the same order: names from the checkpoint's model, shapes from its moments
    ck_names = [n for n, p in ck_model.named_parameters() if p.requires_grad and n != "mu2_table"]
    if ck_names != [n for n, _ in net_params]:
        raise ValueError("--continue-from: the checkpoint's parameters %s... are not this model's %s..."
                         % (ck_names[:3], [n for n, _ in net_params][:3]))
    for k, (n, p) in enumerate(net_params):
        st = optim_state["state"].get(k)
        if st is not None and tuple(st["exp_avg"].shape) != tuple(p.shape):
            raise ValueError("--continue-from: moment %d has shape %s, parameter %s has %s"
                             % (k, tuple(st["exp_avg"].shape), n, tuple(p.shape)))
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    shift = 1 if names and names[0] == "mu2_table" else 0
    grp = dict(optim_state["param_groups"][0], params=list(range(n_nets + shift)))
    return {"state": {k + shift: v for k, v in optim_state["state"].items()}, "param_groups": [grp]}


class GraphStep:
    """step(idxs, features, nsegs) -> (loss, lower_bound): the runner's training step; with --hip-graph (`enabled`) captured
    into a hipGraph on the first batch of the full local size and replayed for the others (a smaller last batch runs eagerly)."""

    def __init__(self, runner, device, local_batch: int, alpha: float, enabled: bool):
        self.runner, self.device, self.bsz, self.alpha, self.enabled = runner, device, local_batch, alpha, enabled
        self.graph = None  # (CUDAGraph, static inputs, static outputs)

    def __call__(self, idxs, features, nsegs):
        idxs = torch.as_tensor(idxs).to(device=self.device, dtype=torch.int64)
        nsegs = torch.as_tensor(nsegs).to(device=self.device, dtype=torch.int64)
        if not self.enabled or features.shape[0] != self.bsz:
            return self.runner.train_step(features, idxs, nsegs, alpha=self.alpha)
        if self.graph is None:
            return self._capture(idxs.clone(), features.clone(), nsegs.clone())
        g, (st_i, st_x, st_n), outs = self.graph
        st_i.copy_(idxs)
        st_x.copy_(features)
        st_n.copy_(nsegs)
        g.replay()
        return outs

    def _capture(self, st_i, st_x, st_n):
        # the warm-up steps and the capture must not train: parameters, Adam moments and the step count are put back
        # afterwards, so this batch gets exactly one update (the first replay) like every other batch
        arenas = [t for o in self.runner.optimizers for t in (o.p_arena.flat, o.m, o.v, o.step_dev)]
        keep = [t.clone() for t in arenas]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):  # warm-up outside the capture (lazy initialisations, allocator pools)
                self.runner.train_step(st_x, st_i, st_n, alpha=self.alpha)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs = self.runner.train_step(st_x, st_i, st_n, alpha=self.alpha)
        self.graph = (g, (st_i, st_x, st_n), outs)
        for t, k in zip(arenas, keep):
            t.copy_(k)
        # capture only RECORDS the kernels: `outs` is uninitialised graph-pool memory until the first replay
        g.replay()
        return outs


def _healthy(runner, say) -> Optional[int]:
    """One host sync: the sticky device words.  Divergence = NaN lower bound in ANY batch since the start
    (fhvae_loss_fwd's nan_flag; the reference tests every batch on the host, train_model.py:464-466).  Recurrence status
    = a persistent bf16 LSTM launch gave up (all 256 CUs were not co-resident): everything computed since is invalid.
    Distributed: the worst code over the ranks, so that every rank stops together.  Returns None, or the exit code 2 / 3."""
    code = runner.check_status()
    if code == 2:
        say("Training diverged")
    elif code == 3:
        say("a persistent LSTM recurrence launch gave up %s: results since are invalid; rerun with FHVAE_NO_CLUSTER=1 if the GPU "
            "is shared" % ("on some rank" if runner.world > 1 else "(status %d)" % runner.lstm_status), file=sys.stderr)
    return code or None


def _dev_bound(model, runner, data, hierarchical: bool):
    """The dev lower bounds of the epoch, a list of tensors.  Hierarchical sampling: dev sequences have no table rows, their mu2
    is estimated like a block's and injected (step 4 of the algorithm; the same on every rank).
    W ranks: [the mean] (a (1,) tensor), every segment counted once: each global dev batch is padded to a multiple of W (the
    padding repeats its first segment; the sharded forward needs equal local sizes), rank r takes the r-th slice, the padding
    is masked out of the sums, and the (sum, count) pair is all-reduced."""
    if hierarchical:
        from hierarchical import estimate_pool_mu2

        pool = data.hs_pools[1]
        kw, num_seqs = {"mu2_table": estimate_pool_mu2(model, pool)}, pool.num_seqs
        batches = pool.epoch(data.args.dev_batch_size, shuffle=False)
    else:
        kw, num_seqs, batches = {}, data.S, data.dev_batches()
    world, rank = runner.world, runner.rank
    if world == 1:
        return [model(features, idxs, num_seqs, nsegs, **kw)[0] for idxs, features, nsegs in batches]
    acc = torch.zeros(2, device=data.device, dtype=torch.float64)
    for idxs, features, nsegs in batches:
        n = features.shape[0]
        per = -(-n // world)
        pos = torch.arange(rank * per, (rank + 1) * per)
        valid = pos < n
        pos = torch.where(valid, pos, torch.zeros_like(pos))
        pick = lambda t: t[pos.to(t.device)]  # noqa: E731
        lb = model(pick(features), pick(torch.as_tensor(idxs)), num_seqs, pick(torch.as_tensor(nsegs)), **kw)[0]
        acc[0] += (lb.double() * valid.to(data.device)).sum()
        acc[1] += int(valid.sum())
    runner.all_reduce_(acc)
    return [(acc[0] / acc[1]).float().reshape(1)]


def _estimate_table(model, runner, data, say):
    """--hierarchical: closed-form mu2 from the current encoder (train_model.py:424-436); unlike the reference the result is
    USED: it initialises the persistent table."""
    from utils import estimate_mu2_dict

    mu2_dict = estimate_mu2_dict(model, data.train_batches(whole=True), data.S)
    rows, row0 = runner.table_rows()[0], runner.row0
    with torch.no_grad():
        for y, v in mu2_dict.items():
            if row0 <= y < row0 + rows.shape[0]:  # every rank has the whole estimate and keeps its own rows
                rows[y - row0] = v
    say(f"hierarchical: mu2 re-estimated for {len(mu2_dict)} of {data.S} sequences")


def _train_epoch(args, runner, data, trainer, step, epoch, say):
    """One epoch of training steps -> (sum of the losses (device), steps, segments trained, exit code or None).  The status
    words are read every --check-interval batches (hierarchical: at the first block end past each interval) and at the end."""
    train_loss, nb, n_seg = torch.zeros((), device=data.device), 0, data.n_train
    data.counts.update(skipped=0, trained=0)
    if trainer is not None:
        checked = [0]

        def block_check(steps):
            if args.check_interval > 0 and steps // args.check_interval > checked[0]:
                checked[0] = steps // args.check_interval
                return _healthy(runner, say)
            return None

        train_loss, nb, n_seg, rc = trainer.run_epoch(epoch, check=block_check)
        if rc is not None:
            return train_loss, nb, n_seg, rc
    else:
        for idxs, features, nsegs in data.train_batches():
            loss, lower_bound = step(idxs, features, nsegs)
            train_loss += loss
            nb += 1
            if args.check_interval > 0 and nb % args.check_interval == 0:
                rc = _healthy(runner, say)
                if rc is not None:
                    return train_loss, nb, n_seg, rc
    return train_loss, nb, n_seg, _healthy(runner, say)  # end of epoch, and before anything is checkpointed


def _train(args, device, world: int, rank: int) -> int:
    say = print if rank == 0 else _quiet  # rank 0 prints (and writes) for all ranks
    import hip_binding as hb
    from hip_optim import FusedAdam, LocalRunner

    # the sticky status words (divergence / a recurrence launch that gave up) are per process: a run starts clean.  After a run
    # that returned 2 or 3 the model it trained is invalid (NaN updates may have been applied until the check interval caught them)
    hb.reset_device_words(device)

    torch.manual_seed(args.seed)
    data = _Data(args, device, world, rank)
    T = args.seg_len
    input_size = T * data.F  # np.prod(example_data.shape), train_model.py:396-398
    hs_K = None
    if args.num_hierarchical_sequences is not None:
        # hierarchical sampling: the table holds one block of K sequences, K clamped to the sequences that have segments
        from hierarchical import hs_clamp

        hs_K = hs_clamp(args.num_hierarchical_sequences, data.seq_counts(), log=say)
    S_model = hs_K if hs_K is not None else data.S  # the table's rows: forward()'s num_seqs
    model = _build_model(args, input_size, S_model, say).to(device)
    if world > 1:
        # data parallel over the batch, the table's rows sharded over the ranks; opt_nets / opt_table replace the one FusedAdam
        from dist_shard import DistributedFHVAE

        runner = DistributedFHVAE(model, lr=args.learning_rate, betas=(args.beta_one, args.beta_two))
    else:
        runner = LocalRunner(model, FusedAdam(model.parameters(), lr=args.learning_rate, betas=(args.beta_one, args.beta_two)),
                             loss_function)
    start_epoch, best_epoch, best_val_lb = (_resume(args, model, runner, S_model, hs_K, input_size, say) if args.continue_from
                                            else (0, 0, -np.inf))
    data.draw()
    if args.sample_hierarchical and hs_K is None:
        _estimate_table(model, runner, data, say)
    if args.exp_dir:
        from utils import save_args, save_checkpoint

        if rank == 0:
            os.makedirs(args.exp_dir, exist_ok=True)
            save_args(args.exp_dir, args)  # train_model.py:422

    step = GraphStep(runner, device, args.training_batch_size // world, args.alpha_dis, args.hip_graph)
    trainer = None
    if hs_K is not None:
        # every block: select its segments, estimate + load its K table rows, one shuffled pass (hierarchical.py)
        from hierarchical import DistributedHierarchicalTrainer, HierarchicalTrainer

        hs_args = (data.hs_pools[0], hs_K, args.training_batch_size, step)
        trainer = (DistributedHierarchicalTrainer(runner, *hs_args, seed=args.seed, log=say) if world > 1 else
                   HierarchicalTrainer(model, runner.optimizer, *hs_args, seed=args.seed, log=say, runner=runner))

    for epoch in range(start_epoch, args.epochs):
        model.train()
        t0 = time.time()
        train_loss, nb, n_seg, rc = _train_epoch(args, runner, data, trainer, step, epoch, say)
        if rc is not None:
            return rc
        dt = time.time() - t0
        if world > 1:
            runner.all_reduce_(train_loss)  # the global loss: the mean of the ranks' (equal-sized) local losses
            train_loss = train_loss / world
            if trainer is None:
                n_seg = data.counts["trained"]
                if data.counts["skipped"]:
                    say("dist: %d segments of the last ragged batch skipped (not a multiple of %d ranks)"
                        % (data.counts["skipped"], world))
            elif trainer.skipped:
                say("dist: %d segments of ragged last batches skipped this epoch (not a multiple of %d ranks)"
                    % (trainer.skipped, world))
                trainer.skipped = 0
        say(f"====> Train set average loss: {train_loss.item() / nb:.4f}  ({n_seg / dt:.0f} segments/s)")
        model.eval()
        with torch.no_grad():
            val_lower_bound = torch.cat(_dev_bound(model, runner, data, trainer is not None))
        say(f"====> Validation set lower bound: {val_lower_bound.mean().item():.4f} "
              f"({val_lower_bound.mean().item() / T:.4f} nats/frame)")
        if check_best(val_lower_bound, best_val_lb):
            best_epoch, best_val_lb = epoch, val_lower_bound.mean().item()
        if args.exp_dir:
            full = runner.state_dict() if world > 1 else None  # (collective: every rank takes part, rank 0 writes)
            if rank == 0:
                save_checkpoint(model, None if world > 1 else runner.optimizer, None,
                                {"val_lower_bound": val_lower_bound.mean().item()}, "run", epoch, best_epoch,
                                val_lower_bound.mean().item(), best_val_lb, args.exp_dir, input_size=input_size,
                                hierarchical_sequences=hs_K, state=full)
        if check_terminate(epoch, best_epoch, args.patience, args.epochs):
            say("Training terminated!")
            break
    say("Training complete!")
    return 0


if __name__ == "__main__":
    sys.exit(main())
