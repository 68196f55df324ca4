"""The grids of the all-pairs kernels are part of the ABI: the chunk of streamed rows per workgroup fixes the layout of the
partials, t-SNE's summation order and the workspace sizes.  The three size functions, swept against their formulas written
out here (the chunk rule of the f32 K5 is tests/disc_plan.py)."""
import pytest

from disc_plan import cdiv as _cdiv, group_bytes as _group_bytes, mfma_chunk as _mfma_chunk

SIZES = list(range(1, 3001)) + [4600, 28000, 100000, 1000000, 1 << 22]
BATCHES = [1, 255, 256, 257, 2048, 16384]
ONE_PASS_CAP = 3 << 29  # 1.5 GiB


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding as hb

    return hb.load_library()


def tsne_ws_bytes(N):
    nxb = _cdiv(N, 256)
    want = max(1, 2048 // nxb)
    chunk = max(512, _cdiv(_cdiv(N, want), 64) * 64)
    nchunks, npad = _cdiv(N, chunk), _cdiv(N, 64) * 64
    return _cdiv((npad + nchunks * 7 * npad + nchunks * nxb * 4) * 4, 256) * 256


def disc_lse_ws_bytes(B, S):
    """(max, sumexp) per (chunk, query): the larger of the VALU kernels' grid (chunks of 8 rows) and the MFMA kernels'"""
    valu_chunk = max(8, _cdiv(_cdiv(S, _cdiv(1024, _cdiv(B, 256))), 8) * 8)
    return max(_cdiv(S, valu_chunk), _cdiv(S, _mfma_chunk(B, S, 1024))) * B * 8


def disc_lse_bwd_ws_bytes(B, S, D):
    """the most 256-query tiles per group (bisection, as the library searches) whose partials fit the cap"""
    if D not in (16, 32) or B * S < 65536:
        return 0
    lo, hi = 0, _cdiv(B, 256)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if _group_bytes(mid, B, S, D) <= ONE_PASS_CAP:
            lo = mid
        else:
            hi = mid - 1
    return _group_bytes(lo, B, S, D) if lo else 0


def test_tsne_workspace(lib):
    bad = [(N, D) for N in SIZES for D in (16, 128) if lib.fhvae_tsne_ws_bytes(N, D) != tsne_ws_bytes(N)]
    assert not bad, bad[:10]
    assert lib.fhvae_tsne_ws_bytes(0, 32) == 0 and lib.fhvae_tsne_ws_bytes((1 << 22) + 1, 32) == 0 and lib.fhvae_tsne_ws_bytes(300, 0) == 0


def test_disc_lse_workspace(lib):
    bad = [(B, S) for B in BATCHES for S in SIZES if lib.fhvae_disc_lse_ws_bytes(B, S) != disc_lse_ws_bytes(B, S)]
    assert not bad, bad[:10]


@pytest.mark.parametrize("D", [16, 32, 64])
def test_disc_lse_bwd_workspace(lib, D):
    bad = [(B, S) for B in BATCHES for S in SIZES if lib.fhvae_disc_lse_bwd_ws_bytes(B, S, D) != disc_lse_bwd_ws_bytes(B, S, D)]
    assert not bad, bad[:10]
