"""The launch plans of the three matrix-product kernels (fhvae_plan_proj, fhvae_plan_wgrad, fhvae_plan_gemm: host-only queries of
the functions the launchers call) against tests/golden/matmul_plans.json, the digests of what the launchers decided before the
plans existed (tests/matmul_plan_sweep.py).  No device is needed."""
import pytest

import matmul_plan_sweep as S

BLOCKS = list(S.load()["digests"])


@pytest.fixture(scope="module")
def cases():
    return S.cases()


def test_golden_names_every_block_of_the_sweep(cases):
    gold = S.load()
    assert list(cases) == BLOCKS == list(gold["calls"]) and len(BLOCKS) == 28
    assert {b: len(c) for b, c in cases.items()} == gold["calls"]


@pytest.mark.parametrize("block", BLOCKS)
def test_plans_reproduce_the_recorded_decisions(cases, block):
    lines = S.rows(block, cases[block])
    assert len(lines) == len(cases[block])
    assert S.digest(lines) == S.load()["digests"][block], "%s: the plans changed; its first lines now:\n%s" % (block, "\n".join(lines[:8]))


def test_sweep_reaches_every_outcome(cases):
    """Every kernel variant, tile, error and grouping outcome occurs in the sweep (a boundary with one side only would not
    notice the boundary moving)."""
    seen, rets = set(), set()
    for block, cs in cases.items():
        if block.startswith("gemm"):
            for dtype, ps in cs[::3] if "x" in block else cs:
                ret, ls = S.gemm_launches(ps, dtype)
                rets.add(ret if ret < 0 else "ok")
                seen |= {(l.variant, l.BM, l.BN, l.CH, l.n > 1) if l.status == 0 else l.status for l in ls}
    tiles = {(64, 64, 8), (64, 64, 32), (128, 128, 16)}
    assert seen >= {(v, bm, bn, ch, False) for v in (1, 2) for bm, bn, ch in tiles} | {(0, 0, 0, 0, False), (3, 64, 64, 32, False), (4, 128, 64, 16, False),
                                                                                      (5, 64, 64, 32, True), (6, 64, 64, 32, True), -2}
    assert rets == {"ok", -2}
    wg = [S.wgrad_launches(S.wgrad_descs(c), bf16)[1] for c, bf16 in cases["wgrad bf16"] + cases["wgrad f32"]]
    assert {l.BN for ls in wg for l in ls} == {128, 256} and {len(ls) for ls in wg} >= {1, 2, 3}
    assert {l.n for ls in wg for l in ls} >= {1, 16} and any(q.shared_c for ls in wg for l in ls for q in l.p[:l.n])
    assert {15, 16} <= {l.grid for ls in wg for l in ls} and {1, 2, 64} <= {l.sk for ls in wg for l in ls}
    assert {S.proj_plan(M, N)[:2] for M, N in cases["proj"]} == {(bm, bn) for bm in S.PROJ_BMS for bn in (128, 256)}
