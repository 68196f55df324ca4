"""The pieces of the training loop that need no GPU: how an epoch's order is cut into batches and over ranks
(train_model._epoch_batches), the same cut inside a hierarchical block (HierarchicalTrainer.estimate / train_pass, driven through
a stub runner, a stub pool and a stub step on CPU tensors; the block's select is a kernel and is replaced by filling seg_ids /
local_idx by hand), and how the status codes of a runner become exit codes and messages (train_model._healthy)."""
import types

import numpy as np
import pytest
import torch

B = 8
HB = 12  # the hierarchical trainer's global batch: it must divide over the ranks (1, 2, 3 and 4 here)


def _ranks(n, world, seed):
    """Per rank: (batches yielded, counts), every rank drawing the same permutation from a generator of its own."""
    from train_model import _epoch_batches

    out = []
    for rank in range(world):
        g = torch.Generator().manual_seed(seed)
        counts = {"skipped": 0, "trained": 0}
        order = lambda m: torch.randperm(m, generator=g)  # noqa: E731
        out.append((list(_epoch_batches(n, B, world, rank, order, lambda sel: sel, counts)), counts))
    return out


@pytest.mark.parametrize("n", [0, 1, 7, 16, 37])
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_epoch_batches_cover_the_permutation_once(world, n):
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5))
    ranks = _ranks(n, world, 5)
    want, skipped = [], 0
    for s0 in range(0, n, B):  # what the ranks train together: the first m - m % W of every global batch
        sel = perm[s0:s0 + B]
        keep = sel.shape[0] - sel.shape[0] % world
        skipped += sel.shape[0] - keep
        if keep:
            want.append(sel[:keep])
    for batches, counts in ranks:
        assert len(batches) == len(want)
        assert counts == {"skipped": skipped, "trained": n - skipped}
        assert [b.shape[0] for b in batches] == [w.shape[0] // world for w in want]  # equal local sizes on every rank
    for k, w in enumerate(want):  # the ranks' slices, in rank order, are the global batch
        assert torch.equal(torch.cat([batches[k] for batches, _ in ranks]), w)
    assert sum(w.shape[0] for w in want) + skipped == n
    if world == 1:
        assert skipped == 0 and (n == 0 or torch.equal(torch.cat(want), perm))


@pytest.mark.parametrize("n", [0, 1, 7, 16, 37])
def test_one_process_order_is_the_global_generators(n):
    from train_model import _epoch_batches

    torch.manual_seed(11)
    got = list(_epoch_batches(n, B, 1, 0, torch.randperm, lambda sel: sel, {"skipped": 0, "trained": 0}))
    torch.manual_seed(11)
    want = torch.randperm(n)
    assert [g.shape[0] for g in got] == [min(B, n - s0) for s0 in range(0, n, B)]
    assert n == 0 or torch.equal(torch.cat(got), want)


class _Pool:
    """40 segments of 5 sequences; features(ids) = the ids themselves."""
    seq_counts = np.array([9, 8, 0, 12, 11])
    num_seqs = 5

    def features(self, ids):
        return ids.clone()

    def batch(self, ids):
        return ids % 5, ids.clone(), ids + 100


class _Est:
    def __init__(self):
        self.added = []

    def add(self, z2, idx):
        self.added.append((z2.tolist(), idx.tolist()))


def _trainer(world, rank, steps, chunk=4):
    from hierarchical import DistributedHierarchicalTrainer

    model = types.SimpleNamespace(pz2=[None, np.float32(0.0)], pmu2=[0.0, np.float32(0.0)], encode_z2=lambda x: x)
    rows = torch.zeros(2, 3)
    runner = types.SimpleNamespace(world=world, rank=rank, model=model, sh=types.SimpleNamespace(S=2), load_label="merge",
                                   table_rows=lambda: (rows, None, None))

    def step(li, x, nsegs):
        steps.append((li.tolist(), x.tolist(), nsegs.tolist()))
        return torch.tensor(float(len(steps))), None

    tr = DistributedHierarchicalTrainer(runner, _Pool(), 2, HB, step, seed=3, chunk=chunk, log=None)
    assert tr.dev == torch.device("cpu") and tr.D == 3 and tr.seg_ids.shape == (23,)  # capacity: the 2 longest sequences
    tr.est = _Est()
    tr.seg_ids[:] = torch.arange(23) * 2 + 1  # (what select would leave: a block's segments and their local table rows)
    tr.local_idx[:] = torch.arange(23) // 12
    return tr


@pytest.mark.parametrize("N", [0, 1, 7, 21, 23])
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_block_estimate_and_pass_on_w_ranks_are_cuts_of_one_process(world, N):
    from dist_shard import rank_range

    one_steps = []
    one = _trainer(1, 0, one_steps)
    one.estimate(N)
    total, nb = one.train_pass(N)
    assert one.skipped == 0 and nb == -(-N // HB) == len(one_steps) and float(total) == sum(range(1, nb + 1))
    # the pass itself: the block's segments in the order of randperm(N) from a generator seeded like the trainer's, in batches of HB
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(3))
    ids = one.seg_ids[perm]
    assert [len(li) for li, _, _ in one_steps] == [min(HB, N - s) for s in range(0, N, HB)]
    assert [v for _, x, _ in one_steps for v in x] == ids.tolist()  # (the stub pool's features are the segment ids)
    assert [v for li, _, _ in one_steps for v in li] == one.local_idx[perm].tolist()
    assert [v for _, _, ns in one_steps for v in ns] == (ids + 100).tolist()
    seen = [v for z2, _ in one.est.added for v in z2]
    assert seen == one.seg_ids[:N].tolist() and all(len(z2) <= 4 for z2, _ in one.est.added)  # every segment once, in chunks
    assert [v for _, li in one.est.added for v in li] == one.local_idx[:N].tolist()

    ranks, rank_steps = [], []
    for r in range(world):
        rank_steps.append([])
        ranks.append(_trainer(world, r, rank_steps[-1]))
        ranks[-1].estimate(N)
        ranks[-1].train_pass(N)
    # estimate: rank r encodes rank_range(N, W, r); the ranges in rank order are the one-process walk
    for r, tr in enumerate(ranks):
        a, b = rank_range(N, world, r)
        assert [v for z2, _ in tr.est.added for v in z2] == one.seg_ids[a:b].tolist()
    assert [v for tr in ranks for z2, _ in tr.est.added for v in z2] == seen
    # pass: every global batch of the one process, cut down to a multiple of W; the ranks' slices in rank order make it up
    want = [(li[:len(li) - len(li) % world], x[:len(x) - len(x) % world], ns[:len(ns) - len(ns) % world]) for li, x, ns in one_steps]
    skipped = sum(len(li) % world for li, _, _ in one_steps)
    want = [w for w in want if w[0]]
    for tr, steps in zip(ranks, rank_steps):
        assert tr.skipped == skipped and len(steps) == len(want)
    for k, w in enumerate(want):
        for field in range(3):
            assert [v for steps in rank_steps for v in steps[k][field]] == w[field]


def test_batch_size_must_divide_over_the_ranks():
    with pytest.raises(ValueError, match="the batch size 8 is not a multiple of the 3 ranks"):
        from hierarchical import DistributedHierarchicalTrainer

        runner = types.SimpleNamespace(world=3, rank=0, model=None, sh=types.SimpleNamespace(S=2))
        DistributedHierarchicalTrainer(runner, _Pool(), 2, B, None)


@pytest.mark.parametrize("world", [1, 2])
def test_healthy_maps_the_status_codes(world):
    from train_model import _healthy

    said = []
    say = lambda *a, **k: said.append((a, sorted(k)))  # noqa: E731
    runner = types.SimpleNamespace(world=world, lstm_status=7, check_status=lambda: code)
    code = 0
    assert _healthy(runner, say) is None and said == []
    code = 2
    assert _healthy(runner, say) == 2 and said.pop() == (("Training diverged",), [])
    code = 3
    assert _healthy(runner, say) == 3
    (text,), kw = said.pop()
    assert kw == ["file"]  # (stderr)
    if world == 1:
        assert text == ("a persistent LSTM recurrence launch gave up (status 7): results since are invalid; rerun with "
                        "FHVAE_NO_CLUSTER=1 if the GPU is shared")
    else:
        assert text == ("a persistent LSTM recurrence launch gave up on some rank: results since are invalid; rerun with "
                        "FHVAE_NO_CLUSTER=1 if the GPU is shared")
