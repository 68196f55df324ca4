"""CPU side of the matrix-product oracle tests (tests/test_gemm_oracle_gpu.py):
  coverage     the library's own launch plans (fhvae_plan_proj / _wgrad / _gemm through tests/matmul_plan_sweep.py) say which
               compiled branch each GPU case reaches; every branch the three launchers can take must be reached by a row of the
               GPU file's case tables (remove a row and this fails);
  sensitivity  the comparator and the canary check reject the errors a kernel could hide, with an f32 emulation (blocked f32
               products, split-K partials added one by one into c0) standing in for the kernel;
  noise floor  the unfaulted emulation stays below the comparator's constants from K = 1 to K = 40960 and 1 to 40 slices;
  fhvae_wgrad_desc_ok at its boundaries (host only: no GPU memory is touched)."""
import ctypes as C

import pytest
import torch

import matmul_plan_sweep as GP
import head_elbo_compare as HC
import test_gemm_oracle_gpu as G
from oracle import gemm_ref as GR


# ---------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------
def test_proj_cases_reach_every_instantiation():
    plans = {(M, N, K): GP.proj_plan(M, N) for M, N, K, _, _ in G.PROJ_CASES}
    for M, N, K, bm, bn in G.PROJ_CASES:
        assert plans[(M, N, K)][:2] == (bm, bn), (M, N, K)
        assert K % 64 == 0 and N % 4 == 0  # proj_eligible
    assert {p[:2] for p in plans.values()} == {(bm, bn) for bm in GP.PROJ_BMS for bn in (128, 256)}
    # every instantiation that fills the chip, in its plain setting: one column tile, one round
    assert {p[:2] for (_, N, _), p in plans.items() if N <= p[1] and p[2] <= 256} >= {(bm, bn) for bm in GP.PROJ_BMS[1:] for bn in (128, 256)}
    tiles = {k: p[2] for k, p in plans.items()}
    full = [t for k, t in tiles.items() if plans[k][:2] == (256, 256)]
    assert 256 in full and any(t < 256 for t in full) and any(t > 512 for t in tiles.values())  # the last single round; three rounds
    assert any(N > 256 and N % 256 == 0 for _, N, _ in plans)                                # two whole column tiles
    assert any(N > 256 and 0 < N % 256 < 16 and tiles[(M, N, K)] > 2 for M, N, K in plans)   # a ragged second one, many row tiles
    res = {(M % p[0], p[0]) for (M, _, _), p in plans.items()}
    assert any(r == 1 for r, _ in res) and any(r == bm - 1 for r, bm in res)  # the last row tile: one row, all but one
    assert {(K // 64) % 2 for _, _, K in plans} == {0, 1}  # the two-stage loop ends on either LDS object


def _wgrad_desc_ok(K, M, N, lda, ldb, ldc, a_col0=0, bf16=True):
    """fhvae_wgrad_desc_ok (bf16 operands); for f32 operands the plan query's own eligibility and the same `ldc >= N`."""
    lib, hb = GP.library()
    d = hb.WgradDesc(GP.P, lda, a_col0, GP.P, ldb, GP.P, ldc, M, N, K)
    return lib.fhvae_wgrad_desc_ok(C.byref(d)) == 1 if bf16 else GP.wgrad_launches([d], False)[0] == 1 and ldc >= N


def _wg_tags(K, M, N, bf16):
    BK = GP.wgrad_elem(bf16)[0]
    (BN, sk, grid, per, _), = GP.wgrad_plan([(K, M, N)], bf16)
    d = per[0]
    t = {"atomic" if d["atomic"] else "plain", "odd slice" if d["ksteps_per"] % 2 else "even slice"}
    if d["last"] < d["ksteps_per"]:
        t.add("short last slice")
    if d["ktail"] in (0, 1, BK - 1):
        t.add("K %% BK = %s" % {0: "0", 1: "1"}.get(d["ktail"], "BK-1"))
    if K < BK:
        t.add("K < BK")
    t.add("grid >= 16, no multiple of 8" if grid >= 16 and grid & 7 else "grid <= 15" if grid <= 15 else "grid other")
    if not d["atomic"] and d["ktail"] and M % GP.WG_BM and N % BN:
        t.add("plain RMW with a K tail, ragged M and N")
    return BN, t


WG_REQUIRED = {"atomic", "plain", "odd slice", "even slice", "short last slice", "K % BK = 0", "K % BK = 1", "K % BK = BK-1", "K < BK",
               "grid >= 16, no multiple of 8", "grid <= 15", "plain RMW with a K tail, ragged M and N"}


@pytest.mark.parametrize("bf16", [True, False])
def test_wgrad_cases_reach_every_branch_in_both_tile_classes(bf16):
    have = {128: set(), 256: set()}
    for K, M, N, _, _ in G.WGRAD_CASES:
        lda, ldb = G.wgrad_lds(M, N)
        assert _wgrad_desc_ok(K, M, N, lda, ldb, N, 0, bf16)
        BN, t = _wg_tags(K, M, N, bf16)
        have[BN] |= t
    for BN in (128, 256):
        assert WG_REQUIRED <= have[BN], (BN, sorted(WG_REQUIRED - have[BN]))
    shapes = [(K, M, N) for K, M, N, _, _ in G.WGRAD_CASES]
    assert any(K == 1 for K, _, _ in shapes)
    assert any(128 < N < 256 for _, _, N in shapes) and any(N > 256 and N % 256 for _, _, N in shapes)
    assert any(M % 8 for _, M, _ in shapes)  # under a padded lda
    for bn in (128, 256):  # ldc > N in each tile class
        assert any(c0 + ex > 0 and (N > 128) == (bn == 256) for _, _, N, c0, ex in G.WGRAD_CASES)


def test_grouped_cases_reach_the_grouping_logic():
    wide, = GP.wgrad_plan(G.GROUPS["wide"], True)
    BN, sk, grid, per, which = wide
    assert (BN, sk, grid) == (256, 4, 36) and grid >= 16 and grid & 7
    assert any(d["clipped"] and d["splitk"] > 1 for d in per)                       # s > ks_total / 2
    assert any(d["splitk"] == 1 and not d["shared_c"] and not d["atomic"] for d in per)  # plain RMW beside split problems
    assert [d["shared_c"] for d in per] == [True, False, False, False, True]
    narrow, = GP.wgrad_plan(G.GROUPS["narrow"], True)
    assert narrow[0] == 128 and narrow[1] > 1 and any(d["clipped"] for d in narrow[3]) and any(d["splitk"] == 1 for d in narrow[3])
    assert any(d["last"] < d["ksteps_per"] for d in narrow[3]) and [d["shared_c"] for d in narrow[3]] == [True, False, False, True]
    both = GP.wgrad_plan(G.GROUPS["both"], True)
    assert [l[0] for l in both] == [256, 128] and [l[1:3] for l in both] == [wide[1:3], narrow[1:3]]
    sev = GP.wgrad_plan(G.GROUPS["seventeen"], True)
    assert [(l[0], len(l[4])) for l in sev] == [(128, 16), (128, 1)]
    assert len({d["ktail"] for l in sev for d in l[3]}) > 8  # heterogeneous K
    for probs in G.GROUPS.values():
        for K, M, N, _ in probs:
            lda, ldb = G.wgrad_lds(M, N)
            assert _wgrad_desc_ok(K, M, N, lda, ldb, N + 7)
    K, D, N = G.PAIR["K"], G.PAIR["D"], G.PAIR["N"]
    assert D == 40 and (2 * D) % 8 == 0 and all(_wgrad_desc_ok(K, D, N, 2 * D + 8, N + 8, N + 7, i * D) for i in range(2))


LINEAR_REQUIRED = {
    "y: LDS-DMA main loop on every tile, both buffers", "y: LDS-DMA main loop on every tile, one panel", "y: LDS-DMA on some tiles, staged on the ragged ones", "y: swapped kernel above 256 tiles",
    "y: 128x128 tiles, ragged, K tail", "y: CH = 8 at K = 64, 16-byte stores", "y: CH = 32 at K = 68", "y: swapped epilogue, scalar stores",
    "y: swapped epilogue, 16-byte stores", "dx: slow kernel", "dw: slow kernel", "dx: mixed-orientation kernel", "dw: one slice",
    "dw: split 2", "dw: split 4 over 2 tiles", "dw: split 4", "dw: split 8",
}


def _linear_tags(M, K, N, relu):
    pl = G.linear_plans(M, K, N, relu)
    t = set()
    (tile, ch, sk, tiles, kernel, dma, vec) = pl["y"]
    assert sk == 1 and kernel != "plain"
    if kernel == "swap+dma" and dma == tiles:
        t.add("y: LDS-DMA main loop on every tile, " + ("both buffers" if K // (ch * 4) >= 2 else "one panel"))
    if kernel == "swap+dma" and 0 < dma < tiles:
        t.add("y: LDS-DMA on some tiles, staged on the ragged ones")
    if kernel == "swap" and tile == (64, 64) and tiles > 256:
        t.add("y: swapped kernel above 256 tiles")
    if tile == (128, 128) and tiles >= 512 and (M % 128 and N % 128) and K % (ch * 4):
        t.add("y: 128x128 tiles, ragged, K tail")
    if ch == 8 and K == 64 and vec:
        t.add("y: CH = 8 at K = 64, 16-byte stores")
    if ch == 32 and K == 68:
        t.add("y: CH = 32 at K = 68")
    t.add("y: swapped epilogue, 16-byte stores" if vec else "y: swapped epilogue, scalar stores")
    for n in ("dx", "dw"):
        if pl[n] == "slow":
            t.add(n + ": slow kernel")
    if pl["dx"] != "slow":
        assert pl["dx"][4] == "plain" and pl["dx"][2] == 1
        t.add("dx: mixed-orientation kernel")
    if pl["dw"] != "slow":
        sk, tiles = pl["dw"][2], pl["dw"][3]
        assert pl["dw"][4] == "plain"
        t.add({1: "dw: one slice", 2: "dw: split 2", 8: "dw: split 8"}.get(sk, "dw: split %d%s" % (sk, " over 2 tiles" if tiles == 2 else "")))
    return t


def test_linear_cases_reach_every_gemm_plan_outcome():
    have = set()
    for M, K, N, kernel, dma, dw_split in G.LINEAR_CASES:
        for relu in (False, True):
            pl = G.linear_plans(M, K, N, relu)
            assert (pl["y"][4], pl["y"][5]) == (kernel, dma), (M, K, N)
            assert pl["dw"] == "slow" or pl["dw"][2] == dw_split, (M, K, N)
            have |= _linear_tags(M, K, N, relu)
    assert have == LINEAR_REQUIRED, (sorted(LINEAR_REQUIRED - have), sorted(have - LINEAR_REQUIRED))
    # the plan's branches that no linear layer takes: bf16 long-K weight gradients and mixed bf16 orientations
    assert GP.gemm_plan(1024, 256, 40960, 0, 0, 1024, 256, auto=True, dtype="bf16")[:4] == ((128, 64), 16, 16, 32)
    assert GP.gemm_plan(64, 64, 64, 1, 0, 64, 64, dtype="bf16") == "slow"
    assert GP.auto_splitk(192, 100) == 1 and GP.auto_splitk(4, 3) == 1 and GP.auto_splitk(1, 1000) == 128


# ---------------------------------------------------------------------------------------------
# an f32 emulation as the "kernel"
# ---------------------------------------------------------------------------------------------
def emulate(a, b, out, BK=64, slices=1, bias=None, fault=None):
    """out[M, N] (f32, holds c0) += A . B^T the way the kernels sum it: a, b KM operands [K, M], [K, N]; f32 products of BK-row
    blocks accumulated in f32, each K slice's partial tile added into `out` in turn (the split-K atomics, in one order).
    fault: None or one of FAULTS."""
    A, B = a.float(), b.float()
    K, M = A.shape
    N = B.shape[1]
    blocks = list(range(0, K, BK))
    per = -(-len(blocks) // slices)
    for s in range(0, len(blocks), per):
        acc = torch.zeros(M, N)
        if s == 0 and bias is not None:
            acc += bias[None, :]
        for k0 in blocks[s:s + per]:
            k1 = min(K, k0 + BK)
            acc = acc + A[k0:k1].t() @ B[k0:k1]
            if fault == "bf16 tile":  # one 64 x 64 tile's accumulator goes through a bf16 rounding
                acc[64:128, 0:64] = acc[64:128, 0:64].bfloat16().float()
            if fault == "k tail twice" and k1 == K:  # one column tile counts the K tail twice
                assert K % BK
                acc[:, 0:64] += A[k0:k1].t() @ B[k0:k1, 0:64]
        if fault == "k row dropped" and s == 0:  # one 16 x 16 block misses one k-row
            acc[16:32, 32:48] -= A[3, 16:32, None] * B[3, None, 32:48]
        out += acc
    if fault == "nan":
        out[5, 7] = float("nan")


FAULTS = ("k row dropped", "bf16 tile", "k tail twice", "nan", "canary")


def _emulated_case(dt, K, M, N, slices, fault=None, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    lda, ldb = G.wgrad_lds(M, N)
    a = G.padded(K, M, lda, 2, G.WG_DTYPES[dt], g, "cpu")
    b = G.padded(K, N, ldb, 2, G.WG_DTYPES[dt], g, "cpu")
    c, full, c0 = G.canary(M, N, 1, 3, 4, "cpu", gen=g)
    emulate(a, b, c, BK=64 if dt == "bf16" else 32, slices=slices, fault=fault)
    if fault == "canary":
        full[1 + M, 3] = 0.0  # the first element of the row after the output
    want, ab = GR.contraction(a, b, False, False, c0=c0)
    log = []
    bad = HC.check_contraction(c, want, ab, K, HC.HEAD[dt], "emulated %s K %d" % (dt, K), quiet=True, log=log)
    return bad + G.canary_bad(c, full, "emulated"), log[0][1]


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("fault", FAULTS)
def test_comparator_rejects_each_fault(dt, fault):
    clean, _ = _emulated_case(dt, 200, 128, 192, 2)
    assert not clean, clean
    bad, st = _emulated_case(dt, 200, 128, 192, 2, fault=fault)
    assert bad, (fault, st)
    if fault in FAULTS[:3]:  # far above the limits, not at their edge
        k = HC.HEAD[dt]
        worst = max(st["max"] / k["cmax"], max(bm / (HC.LOCAL_RATIO * bd + k["cbin"]) for bm, bd in st["bins"].values()))
        assert worst > 30, (fault, worst)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_noise_floor_is_below_the_constants(dt):
    worst = {"max": 0.0, "mean": 0.0, "bin": 0.0}
    for K, slices in [(1, 1), (2, 1), (7, 1), (63, 1), (64, 1), (200, 2), (1000, 7), (4096, 40), (40960, 1), (40960, 40)]:
        bad, st = _emulated_case(dt, K, 128, 192, slices, seed=K + slices)
        assert not bad, (K, slices, bad)
        worst["max"], worst["mean"] = max(worst["max"], st["max"]), max(worst["mean"], st["mean"])
        worst["bin"] = max(worst["bin"], max(bm / max(bd, 1e-30) for bm, bd in st["bins"].values()))
    print("noise floor %s: max %.2f mean %.2f worst bin / median %.2f" % (dt, worst["max"], worst["mean"], worst["bin"]))
    k = HC.HEAD[dt]
    assert worst["max"] <= k["cmax"] / 2 and worst["mean"] <= k["cmean"] and worst["bin"] <= 2.0


# ---------------------------------------------------------------------------------------------
# fhvae_wgrad_desc_ok (csrc/lstm.hip wg_from_desc -> csrc/wgrad.hip wgrad_eligible)
# ---------------------------------------------------------------------------------------------
def test_wgrad_desc_ok_at_its_boundaries():
    lib, hb = GP.library()
    P = GP.P  # a 16-byte aligned address; nothing is dereferenced

    def ok(K, M, N, lda, ldb, ldc, a_col0=0, a=P):
        d = hb.WgradDesc(a, lda, a_col0, P, ldb, P, ldc, M, N, K)
        got = lib.fhvae_wgrad_desc_ok(C.byref(d))
        # the plan query refuses what the launcher refuses: the same rule, without wg_from_desc's `ldc >= N`
        assert bool(got) == (GP.wgrad_launches([d], True)[0] == 1 and ldc >= N), (K, M, N, lda, ldb, ldc, a_col0)
        return got

    K30 = (1 << 30) // (512 * 2)  # K lda 2 == 2^30 at lda = 512
    assert ok(K30 - 1, 256, 8, 512, 8, 8) == 1 and ok(K30, 256, 8, 512, 8, 8) == 0
    assert ok(K30 - 1, 8, 256, 8, 512, 256) == 1 and ok(K30, 8, 256, 8, 512, 256) == 0  # ... and the same for K ldb 2
    assert ok(64, 40, 72, 80, 72, 72, a_col0=40) == 1 and ok(64, 40, 72, 72, 72, 72, a_col0=40) == 0  # lda below a_col0 + M ...
    assert ok(64, 40, 72, 79, 72, 72, a_col0=40) == 0  # ... and one short of it
    assert ok(64, 40, 72, 80, 72, 72) == 1 and ok(64, 40, 72, 80, 72, 71) == 0  # ldc < N
    assert ok(64, 40, 72, 84, 72, 72) == 0 and ok(64, 40, 72, 80, 72, 72, a=P + 8) == 0  # lda % 8, a base off 16 bytes
    assert ok(64, 40, 72, 80, 72, 72, a_col0=-8) == 0 and ok(0, 40, 72, 80, 72, 72) == 0
