"""The block merge of distributed hierarchical sampling on a MI355X (fhvae_hs_pack_partials, fhvae_mu2_merge_load_shard)
against the numpy model of tests/hs_merge_ref.py: bit for bit against its float32 rank-order emulation, within 1e-6 relative
of float64; the Adam moment rows zeroed inside the shard only; the accumulators cleared; repeatable."""
import numpy as np
import pytest
import torch

from hs_merge_ref import merge_rows_f32, merge_rows_f64, pack, shard_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hb():
    import hip_binding as hb

    hb.load_library()
    return hb


def _partials(W, K, D, seed):
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 50, size=(W, K)).astype(np.float32)
    cnt[rng.random((W, K)) < 0.3] = 0
    cnt[:, K // 2] = 0  # a row no rank saw
    zsum = (rng.standard_normal((W, K, D)) * (1 + cnt[..., None])).astype(np.float32)
    zsum[cnt == 0] = 0
    return zsum, cnt


@pytest.mark.parametrize("W", [1, 2, 3, 4])
@pytest.mark.parametrize("K,D", [(7, 16), (5000, 32), (3, 8)])
def test_pack_and_merge_load_against_oracles(hb, W, K, D):
    dev = torch.device("cuda")
    ratio = 0.25
    zsum, cnt = _partials(W, K, D, 100 * W + K)
    # pack: every rank's accumulators -> (K, D+1), accumulators cleared
    packed = []
    for w in range(W):
        zs, c = torch.from_numpy(zsum[w]).to(dev), torch.from_numpy(cnt[w]).to(dev)
        out = torch.full((K, D + 1), -3.0, device=dev)
        hb.hs_pack_partials(zs, c, out)
        packed.append(out)
        assert np.array_equal(out.cpu().numpy(), pack(zsum[w], cnt[w]))
        assert not zs.any() and not c.any()
    parts = torch.stack(packed).contiguous()
    parts_h = parts.cpu().numpy()
    for r in range(W):  # (W = 3 with K = 3: one row each; K = 7, W = 4: ragged last shard)
        a, b = shard_rows(K, W, r)
        n = b - a
        shard = torch.full((max(n, 0), D), 9.0, device=dev)
        m_all = torch.full((K, D), 5.0, device=dev)
        v_all = torch.full((K, D), 7.0, device=dev)
        hb.mu2_merge_load_shard(parts, a, b, shard, m_all[a:b], v_all[a:b], ratio)
        got = shard.cpu().numpy()
        assert np.array_equal(got, merge_rows_f32(parts_h, a, b, ratio))  # bit for bit
        want = merge_rows_f64(parts_h, a, b, ratio)
        # relative to the magnitude of the terms (the partials can cancel): the float32 rounding of W - 1 adds and a division
        scale = merge_rows_f64(np.abs(parts_h), a, b, ratio)
        assert np.all(np.abs(got - want) <= 1e-6 * scale), np.max(np.abs(got - want) / np.maximum(scale, 1e-30))
        m_h, v_h = m_all.cpu().numpy(), v_all.cpu().numpy()
        assert (m_h[a:b] == 0).all() and (v_h[a:b] == 0).all()
        assert (np.delete(m_h, np.s_[a:b], axis=0) == 5.0).all() and (np.delete(v_h, np.s_[a:b], axis=0) == 7.0).all()
        # repeatable: the same inputs give the same bits
        again = torch.empty_like(shard)
        hb.mu2_merge_load_shard(parts, a, b, again, torch.empty_like(shard), torch.empty_like(shard), ratio)
        assert torch.equal(again, shard)


def test_empty_shard_launches_nothing(hb):
    """K = 1 over W = 2: rank 1 owns no row; the call is a no-op on empty buffers."""
    dev = torch.device("cuda")
    parts = torch.rand(2, 1, 5, device=dev)
    a, b = shard_rows(1, 2, 1)
    assert (a, b) == (1, 1)
    e = torch.empty(0, 4, device=dev)
    hb.mu2_merge_load_shard(parts, a, b, e, e.clone(), e.clone(), 0.25)
    torch.cuda.synchronize()
    one = torch.empty(1, 4, device=dev)
    hb.mu2_merge_load_shard(parts, 0, 1, one, torch.ones(1, 4, device=dev), torch.ones(1, 4, device=dev), 0.25)
    assert np.array_equal(one.cpu().numpy(), merge_rows_f32(parts.cpu().numpy(), 0, 1, 0.25))
