"""CPU checks of the distributed mode of train_model.py and of distributed hierarchical sampling: how global batches and a
block's estimate are cut over ranks, the argument refusals, the numpy model of the rank-order block merge, and the host-side
argument checks of the two merge entry points."""
import ctypes

import numpy as np
import pytest

from hs_merge_ref import merge_rows_f32, merge_rows_f64, pack, shard_rows


@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("n", [0, 1, 7, 8, 13, 64, 256])
def test_rank_slices_partition_the_batch_and_drop_at_most_w_minus_1(world, n):
    from dist_shard import rank_slice

    covered, skipped = [], set()
    for r in range(world):
        a, b, skip = rank_slice(n, world, r)
        assert 0 <= a <= b <= n and b - a == n // world  # equal local sizes on every rank
        covered.extend(range(a, b))
        skipped.add(skip)
    assert skipped == {n % world} and n % world <= world - 1
    # the slices are contiguous, disjoint and in rank order; together they are the batch minus its tail
    assert covered == list(range(n - n % world))


def test_tail_rule_on_an_epoch():
    """A full batch (B a multiple of W) is never cut; only the epoch's last ragged batch loses its n % W tail."""
    from dist_shard import rank_slice

    B, W, n_train = 12, 4, 103
    trained = skipped = 0
    for s0 in range(0, n_train, B):
        n = min(B, n_train - s0)
        a, b, skip = rank_slice(n, W, 0)
        if n == B:
            assert skip == 0 and b - a == B // W
        trained += (b - a) * W
        skipped += skip
    assert (trained, skipped) == (100, 3)


@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
def test_estimate_ranges_cover_every_block_segment_once(world):
    from dist_shard import rank_range

    rng = np.random.default_rng(world)
    counts = rng.integers(0, 30, size=9)
    local_idx = np.repeat(np.arange(9), counts)  # a block's CSR list: local indices non-decreasing
    N = local_idx.shape[0]
    zs = rng.standard_normal((N, 3))
    hits = np.zeros(N, np.int64)
    total, n = np.zeros((9, 3)), np.zeros(9)
    for r in range(world):
        a, b = rank_range(N, world, r)
        hits[a:b] += 1
        np.add.at(total, local_idx[a:b], zs[a:b])  # each rank's partial over its range ...
        np.add.at(n, local_idx[a:b], 1)
    assert (hits == 1).all()
    # ... summed over the ranks: the whole block, also for sequences that cross a range boundary
    want = np.zeros((9, 3))
    np.add.at(want, local_idx, zs)
    np.testing.assert_allclose(total, want, rtol=1e-12, atol=1e-12)
    assert np.array_equal(n, counts)
    if world > 1:
        crossing = [local_idx[rank_range(N, world, r)[0] - 1] == local_idx[rank_range(N, world, r)[0]]
                    for r in range(1, world) if 0 < rank_range(N, world, r)[0] < N]
        assert any(crossing) or world >= N  # (the case is really exercised for these counts)


def test_dist_argument_refusals(monkeypatch, capsys):
    import train_model

    p = train_model.build_parser()
    assert "not a multiple of the 4 ranks" in train_model.dist_arg_error(p.parse_args(["--training-batch-size", "10"]), 4)
    assert train_model.dist_arg_error(p.parse_args(["--training-batch-size", "12"]), 4) is None
    msg = train_model.dist_arg_error(p.parse_args(["--training-batch-size", "8", "--hip-graph", "--dist-backend", "gloo"]), 2)
    assert "--hip-graph" in msg and "nccl" in msg
    assert train_model.dist_arg_error(p.parse_args(["--training-batch-size", "8", "--hip-graph"]), 2) is None
    assert p.parse_args([]).dist_backend == "nccl"
    with pytest.raises(SystemExit):
        p.parse_args(["--dist-backend", "mpi"])
    # main() refuses before it touches a process group or a GPU
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert train_model.main(["--training-batch-size", "7"]) == 1
    assert "not a multiple of the 2 ranks" in capsys.readouterr().err
    assert train_model.main(["--training-batch-size", "8", "--hip-graph", "--dist-backend", "gloo"]) == 1
    assert "--hip-graph in distributed mode needs --dist-backend nccl" in capsys.readouterr().err


def test_merge_model_against_the_definition():
    rng = np.random.default_rng(0)
    W, K, D, ratio = 3, 7, 5, 0.25
    zsum = rng.standard_normal((W, K, D)).astype(np.float32)
    cnt = rng.integers(0, 4, size=(W, K)).astype(np.float32)
    cnt[:, 2] = 0  # a row no rank saw
    parts = np.stack([pack(zsum[w], cnt[w]) for w in range(W)])
    assert parts.shape == (W, K, D + 1) and np.array_equal(parts[1, :, D], cnt[1])
    for r in range(W):
        a, b = shard_rows(K, W, r)
        got = merge_rows_f32(parts, a, b, ratio)
        want = merge_rows_f64(parts, a, b, ratio)
        assert got.shape == (b - a, D) and got.dtype == np.float32
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7)
        if a <= 2 < b:
            assert (got[2 - a] == 0).all()
    # the rank order is the summation order: ((p0 + p1) + p2) in float32
    p = np.array([[[1e8, 1.0]], [[1.0, 1.0]], [[-1e8, 1.0]]], np.float32)
    assert merge_rows_f32(p, 0, 1, 0.0)[0, 0] == np.float32(0.0)  # 1e8 + 1 rounds back to 1e8
    assert shard_rows(7, 2, 1) == (4, 7) and shard_rows(1, 2, 1) == (1, 1)


def test_merge_entry_points_check_arguments_on_the_host():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding as hb

    lib = hb.load_library()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.fhvae_hs_pack_partials(None, p, p, 2, 3, None) == -1
    assert lib.fhvae_hs_pack_partials(p, p, p, 0, 3, None) == -2
    assert lib.fhvae_mu2_merge_load_shard(None, 2, 4, 0, 2, p, p, p, 3, 0.25, None) == -1
    assert lib.fhvae_mu2_merge_load_shard(p, 2, 4, 3, 2, p, p, p, 3, 0.25, None) == -2   # row1 < row0
    assert lib.fhvae_mu2_merge_load_shard(p, 2, 4, 0, 5, p, p, p, 3, 0.25, None) == -2   # row1 > K
    assert lib.fhvae_mu2_merge_load_shard(p, 0, 4, 0, 2, p, p, p, 3, 0.25, None) == -2   # W = 0
    assert lib.fhvae_mu2_merge_load_shard(p, 2, 4, 0, 2, None, p, p, 3, 0.25, None) == -1
    # an empty shard (more ranks than rows) launches nothing: OK without touching a GPU, even without row buffers
    assert lib.fhvae_mu2_merge_load_shard(p, 2, 1, 1, 1, None, None, None, 3, 0.25, None) == 0
