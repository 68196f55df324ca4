"""csrc/proj.hip's operand rings (NSA slots of the A operand, NSB of the B operand, counted waits) against the float64 oracle
(oracle/gemm_ref.py), with the comparator, the constants and the buffers of tests/test_gemm_oracle_gpu.py: HEAD["bf16"] through
head_elbo_compare.check_contraction, NaN-padded leading dimensions (lda, ldb > K), a sentinel-filled output.

A ring that is refilled too early, read too early or waited for with the wrong count gives a wrong or a run-dependent product at
the k-steps where it fills, wraps and wraps once more, so every K / 64 in RING_NK runs: every depth up to 8 at those boundaries,
past the period of the deepest ring pair (12 steps at (4, 3)) and of two periods.  The tiles:
  BM = 64  (M = 65):     8 A pieces per stage, one per wave; rings (4, 3)
  BM = 96  (M = 16391): 12 A pieces: waves 0-3 have a second one, waves 4-7 send a padding piece into the dump; rings (4, 3)
  BM = 160 (M = 32775): the bench tile, 20 A pieces (3 / 2 + a padding piece per wave); rings (3, 3) at BN = 256
each with BN = 128 (N = 4, 128) and BN = 256 (N = 160, 256), without a bias, with one, and at N = 160 with the two-vector bias of
the decoder's head pair (fhvae_gauss_head_pair_fwd, the one entry point that reaches it: its weight operand has ldb = K).

Measured on an MI355X (every case of this file; ratio to U sqrt(K) absprod, bound cmax = 4): max 0.27 (16391 x 160 x 64, BM 96,
split bias) / mean 0.0055; the bench tile's rows against the device product max 0.25.  The outputs are bit-identical to those of
the two-stage kernel this replaced (tools/exp/ab_proj_bits.py, profiles/proj_ring_bit_identity.txt).
"""
import math

import pytest
import torch

import head_elbo_compare as HC
import matmul_plan_sweep as GP
from oracle import gemm_ref as GR
from test_gemm_oracle_gpu import _gen, canary, canary_bad, padded

pytestmark = pytest.mark.gpu

RING_NK = [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 33]
RING_M = {65: 64, 16391: 96}  # M -> BM
RING_N = [4, 128, 160, 256]
BENCH_M = 32775               # the smallest M class that plans BM = 160
BENCH_NK = [(256, 1024), (160, 256), (256, 192)]  # the from-above term, the head forward, the head's dh


@pytest.fixture(scope="module")
def hb():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding

    hip_binding.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return hip_binding


def _run(hb, a, b, out, mode, g):
    """One launch into `out`; returns (bias for the oracle or None)."""
    N = b.shape[0]
    if mode == "none":
        hb.proj_bf16(a, b, None, out=out)
        return None
    if mode == "bias":
        bv = torch.randn(N, generator=g).cuda()
        hb.proj_bf16(a, b, bv, out=out)
        return bv
    D = N // 2  # "split": columns [0, D) take b_mu, [D, 2 D) take b_lv
    b_mu, b_lv = torch.randn(D, generator=g).cuda(), torch.randn(D, generator=g).cuda()
    assert b.stride(0) == b.shape[1]
    hb._call("fhvae_gauss_head_pair_fwd", a.data_ptr(), a.stride(0), b.data_ptr(), b_mu.data_ptr(), b_lv.data_ptr(), out.data_ptr(),
             out.stride(0), a.shape[0], a.shape[1], D)
    return torch.cat([b_mu, b_lv])


@pytest.mark.parametrize("nk", RING_NK)
@pytest.mark.parametrize("N", RING_N)
@pytest.mark.parametrize("M", sorted(RING_M))
def test_ring_fill_wrap_and_wrap_plus_one(hb, M, N, nk):
    K = 64 * nk
    assert GP.proj_plan(M, N)[:2] == (RING_M[M], 256 if N > 128 else 128)
    bad = []
    for mode in ["none", "bias"] + (["split"] if N == 160 else []):
        g = _gen(11, M, N, K, len(mode))
        a = padded(M, K, K + 8, 3, torch.bfloat16, g, "cuda")
        b = padded(N, K, K if mode == "split" else K + 16, 2, torch.bfloat16, g, "cuda")
        out, full, _ = canary(M, N, 1, 4, 4, "cuda")
        bv = _run(hb, a, b, out, mode, g)
        want, ab = GR.contraction(a, b, True, True, bias=bv)
        label = "proj ring %dx%dx%d BM %d %s" % (M, N, K, RING_M[M], mode)
        bad += HC.check_contraction(out, want, ab, K, HC.HEAD["bf16"], label) + canary_bad(out, full, label)
    assert not bad, bad


@pytest.fixture(scope="module")
def bench_tile(hb):
    """(N, K) -> (a, b, out, full) of one launch per bench shape at M = BENCH_M, shared by the tests below and left unchanged."""
    runs = {}
    for N, K in BENCH_NK:
        assert GP.proj_plan(BENCH_M, N)[:2] == (160, 256)
        g = _gen(12, BENCH_M, N, K)
        a = padded(BENCH_M, K, K + 8, 3, torch.bfloat16, g, "cuda")
        b = padded(N, K, K + 16, 2, torch.bfloat16, g, "cuda")
        out, full, _ = canary(BENCH_M, N, 1, 4, 4, "cuda")
        hb.proj_bf16(a, b, None, out=out)
        runs[(N, K)] = (a, b, out, full)
    return runs


@pytest.mark.parametrize("N,K", BENCH_NK)
def test_bench_tile_against_the_oracle_and_the_device_product(hb, bench_tile, N, K):
    """Whole row tiles 0, 1, a middle one and the ragged last one (4 of 205; every tile runs the same code) against the float64
    oracle; every other row against the device's own f32 product under the same per-element bound, cmax U sqrt(K) absprod."""
    a, b, out, full = bench_tile[(N, K)]
    M, BM = BENCH_M, 160
    tiles = -(-M // BM)
    rows = torch.cat([torch.arange(t * BM, min((t + 1) * BM, M)) for t in (0, 1, tiles // 2, tiles - 1)]).cuda()
    label = "proj bench tile %dx%dx%d" % (M, N, K)
    want, ab = GR.contraction(a[rows], b, True, True)
    bad = HC.check_contraction(out[rows], want, ab, K, HC.HEAD["bf16"], label + " (oracle rows)") + canary_bad(out, full, label)
    rest = torch.ones(M, dtype=torch.bool, device="cuda")
    rest[rows] = False
    assert int(rest.sum()) == M - rows.numel() > 0
    af, bf = a[rest].float(), b.float()
    ref, ab = (af @ bf.t()).double(), (af.abs() @ bf.abs().t()).double()
    den = HC.U * math.sqrt(K) * ab + HC._floor(ab, HC.U * math.sqrt(K))
    st = HC.measure(out[rest], ref, den)
    print("%-40s %s" % (label + " (device rows)", HC.fmt(st)))
    if not st["finite"]:
        bad.append(label + ": not finite")
    if st["max"] > HC.HEAD["bf16"]["cmax"]:
        bad.append("%s: max %.3g of the bound on the rows against the device product" % (label, st["max"]))
    assert not bad, bad


@pytest.mark.parametrize("M,N,K", [(16391, 160, 64 * 17), (BENCH_M, 256, 1024)])
def test_two_calls_are_bit_identical(hb, M, N, K):
    """No atomics and no order that depends on timing: a ring read before its DMA landed would differ from run to run."""
    g = _gen(13, M, N, K)
    a = padded(M, K, K + 8, 3, torch.bfloat16, g, "cuda")
    b = padded(N, K, K + 16, 2, torch.bfloat16, g, "cuda")
    outs = [hb.proj_bf16(a, b, None, out=canary(M, N, 1, 4, 4, "cuda")[0]) for _ in range(2)]
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
