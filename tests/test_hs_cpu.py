"""CPU checks of hierarchical sampling (hierarchical.py, csrc/hs.hip): the C entry points are declared, exported and bound and
reject bad arguments on the host; the block planner; the CSR over a pool's sequences; the CLI flag."""
import os
import re

import numpy as np
import pytest

from test_data_ckpt_cpu import corpus  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fhvae_hs_select", "fhvae_mu2_accumulate_sorted", "fhvae_mu2_load_table")


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding as hb

    return hb.load_library()


def test_symbols_declared_exported_bound(lib):
    import hip_binding as hb

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fhvae_hip.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(lib, n) and n in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12


def test_argument_errors_on_the_host(lib):
    # NULL pointers / non-positive shapes: FHVAE_ERR_NULL (-1) / FHVAE_ERR_SHAPE (-2), before any launch
    assert lib.fhvae_hs_select(None, 4, None, 2, None, None, None, 8, None, None) == -1
    assert lib.fhvae_mu2_accumulate_sorted(None, None, None, None, 4, 2, 8, None, None) == -1
    assert lib.fhvae_mu2_load_table(None, None, None, None, None, 2, 8, 0.25, None) == -1
    p = 64  # (a non-NULL address that is never dereferenced: the shape checks come first)
    assert lib.fhvae_hs_select(p, 0, p, 2, p, p, p, 8, p, None) == -2
    assert lib.fhvae_hs_select(p, 4, p, 0, p, p, p, 8, p, None) == -2
    assert lib.fhvae_hs_select(p, 4, p, 2, p, p, p, -1, p, None) == -2
    assert lib.fhvae_mu2_accumulate_sorted(p, p, p, p, 4, 2, 0, p, None) == -2
    assert lib.fhvae_mu2_accumulate_sorted(p, p, p, p, 4, 2, 257, p, None) == -5  # D > 256: FHVAE_ERR_LIMIT
    assert lib.fhvae_mu2_load_table(p, p, p, p, p, 0, 8, 0.25, None) == -2


def _check_plan(plan, eligible, K):
    eligible = set(int(e) for e in eligible)
    assert plan.shape == (-(-len(eligible) // K), K)
    for row in plan:
        assert len(set(row.tolist())) == K                  # K distinct sequences per block
        assert set(row.tolist()) <= eligible                # only eligible sequences
    flat = plan.reshape(-1).tolist()
    first = flat[: len(eligible)]
    assert sorted(first) == sorted(eligible)                # every eligible sequence once per epoch ...
    topup = flat[len(eligible):]                            # ... plus the top-up of the last block
    assert len(topup) == plan.size - len(eligible)
    last = plan[-1].tolist()
    assert not set(topup) & set(last[: K - len(topup)])


@pytest.mark.parametrize("S,K", [(10, 3), (10, 5), (10, 1), (1000, 257), (7, 7)])
def test_planner_blocks(S, K):
    from hierarchical import eligible_sequences, plan_epoch

    counts = np.random.default_rng(S).integers(0, 4, size=S)
    counts[:K] = 1  # at least K eligible
    el = eligible_sequences(counts)
    assert np.array_equal(el, np.flatnonzero(counts > 0))
    plan = plan_epoch(el, K, seed=3, epoch=1)
    _check_plan(plan, el, K)
    assert np.array_equal(plan, plan_epoch(el, K, seed=3, epoch=1))        # same seed and epoch: same plan
    assert not np.array_equal(plan_epoch(el, K, 3, 1).ravel()[: len(el)], plan_epoch(el, K, 3, 2).ravel()[: len(el)]) or len(el) < 3


def test_planner_k_at_least_s_and_empty_sequences():
    from hierarchical import eligible_sequences, hs_clamp, plan_epoch

    counts = np.array([3, 0, 2, 0, 1])
    el = eligible_sequences(counts)
    assert el.tolist() == [0, 2, 4]                         # sequences with no segments are never drawn
    lines = []
    K = hs_clamp(10, counts, log=lines.append)
    assert K == 3 and len(lines) == 1 and "clamped" in lines[0]
    plan = plan_epoch(el, K, 0, 0)
    assert plan.shape == (1, 3) and sorted(plan[0].tolist()) == [0, 2, 4]   # K >= S: one block
    for seed in range(20):
        for epoch in range(3):
            assert not set(plan_epoch(el, 2, seed, epoch).ravel().tolist()) & {1, 3}
    with pytest.raises(ValueError):
        plan_epoch(el, 4, 0, 0)
    with pytest.raises(ValueError):
        hs_clamp(3, np.zeros(4))


def test_csr_on_the_corpus(corpus):
    import datasets as D

    root, _ = corpus
    ds = D.NumpyDataset(root / "feats.scp", root / "len.scp", min_len=20, seg_len=20, seg_shift=8)
    seq_of = np.array([ds.seq2idx[s.seq] for s in ds.segs])
    counts, ptr = D.seq_csr(ds.seq_nsegs, seq_of)
    assert counts.tolist() == [5, 1, 15] and ptr.tolist() == [0, 5, 6, 21]
    for s in range(3):
        assert (seq_of[ptr[s]:ptr[s + 1]] == s).all()
    with pytest.raises(ValueError):
        D.seq_csr(ds.seq_nsegs, seq_of[::-1])                # not grouped in sequence order
    assert D.seq_csr([2, -1, 1], [0, 0, 2])[1].tolist() == [0, 2, 2, 3]   # make_segs' negative count = no segments


def test_cli_flag():
    import train_model as TM

    a = TM.build_parser().parse_args(["--num-hierarchical-sequences", "5000"])
    assert a.num_hierarchical_sequences == 5000 and not a.sample_hierarchical
    b = TM.build_parser().parse_args(["--hierarchical"])
    assert b.sample_hierarchical and b.num_hierarchical_sequences is None
    c = TM.build_parser().parse_args([])
    assert vars(b) == dict(vars(c), sample_hierarchical=True)
