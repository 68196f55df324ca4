"""CPU checks behind tests/test_glue_gpu.py: (1) every oracle of tests/glue_ref.py against an independent torch-CPU expression
on the case tables of tests/glue_cases.py, the tables the GPU file runs; (2) the tables and comparators reject plausible wrong
kernels, written here as numpy functions; (3) the argument errors of the entry points, which return before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import glue_cases as G
import glue_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def eq_bits(a, b):
    return np.array_equal(G.bits(a), G.bits(np.asarray(b)))


# ---------------------------------------------------------------------------------------------
# 1. the oracles against torch-CPU expressions
# ---------------------------------------------------------------------------------------------
def test_segment_gather_ref_against_torch():
    for c in G.segment_gather_cases():
        pool, start = t(c["pool"]), t(c["start"])
        fr = start[:, None] + torch.arange(c["T"])[None, :]
        ok = (fr >= 0) & (fr < pool.shape[0])
        x = pool[fr.clamp(0, pool.shape[0] - 1)]
        if c["mean"] is not None:
            x = (x - t(c["mean"])) * t(c["inv_std"])
        x = torch.where(ok[..., None], x, torch.zeros(()))
        btf, tbf, oob = R.segment_gather_ref(c["pool"], c["start"], c["T"], c["mean"], c["inv_std"])
        assert eq_bits(btf, x.numpy()) and eq_bits(tbf, x.transpose(0, 1).contiguous().numpy()), c["name"]
        assert oob == int((~ok).any()) == int(c["name"].endswith("all"))


def test_accumulate_and_finalize_ref_against_torch():
    for c in G.accumulate_cases():
        z, idx, S = t(c["z"]).double(), t(c["idx"]), c["S"]
        keep = (idx >= 0) & (idx < S)
        want = torch.zeros(S, c["D"], dtype=torch.float64).index_add_(0, idx[keep], z[keep])
        wabs = torch.zeros(S, c["D"], dtype=torch.float64).index_add_(0, idx[keep], z[keep].abs())
        zsum, absum, cnt = R.mu2_accumulate_ref(c["z"], c["idx"], S)
        assert np.allclose(zsum, want.numpy(), rtol=1e-13, atol=1e-12) and np.allclose(absum, wabs.numpy(), rtol=1e-13)
        assert np.array_equal(cnt, torch.bincount(idx[keep], minlength=S).numpy())
        if c["N"] > 1:
            assert (cnt == 0).any() or S == 4, c["name"]  # some ids never occur
            assert (~keep).sum() >= 6                      # -1 and S are among the rows
    for c in G.finalize_cases():
        zs, n = t(c["zsum"]), t(c["cnt"])
        want = torch.where(n[:, None] > 0, zs / (n[:, None] + torch.tensor(c["ratio"], dtype=torch.float32)), torch.zeros_like(zs))
        assert eq_bits(R.mu2_finalize_ref(c["zsum"], c["cnt"], c["ratio"]), want.numpy()), c["name"]
        assert (c["cnt"] == 0).any() or c["S"] == 1


def test_layout_refs_against_torch():
    for c in G.to_time_major_cases():
        assert eq_bits(R.to_time_major_ref(c["x"]), t(c["x"]).transpose(0, 1).contiguous().numpy()), c["name"]
    for c in G.cast_cases() + [G.cast_denormal_case()]:
        want = t(c["x"]).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        got = R.bf16_rne(c["x"])
        G.same_bf16(got, want, c["name"])  # (torch keeps a NaN's upper payload bits; both are NaN)
        assert np.array_equal(R.bf16_is_nan(got), np.isnan(c["x"]))
    # the named edges, by hand
    e = R.bf16_rne(G.CAST_EDGE_BITS.view(F32))
    assert list(e[:9]) == [0x0000, 0x8000, 0x3F80, 0x3F82, 0x3F81, 0x7F7F, 0x7F80, 0x7F80, 0xFF80] and R.bf16_is_nan(e[9:12]).all()
    d = R.bf16_rne(G.CAST_DENORMAL_BITS[:2].view(F32))
    assert list(d) == [0x0000, 0x0002]  # 0x00008000: a tie, down to even; 0x00018000: a tie, up to even


def test_gather_ref_against_torch():
    for c in G.gather_cases():
        s = t(c["idx"]) - c["off"]
        ok = (s >= 0) & (s < c["table"].shape[0])
        want = torch.where(ok[:, None], t(c["table"])[s.clamp(0, c["table"].shape[0] - 1)], torch.zeros(()))
        got, oob = R.gather_fwd_ref(c["table"], c["idx"], c["off"])
        assert eq_bits(got, want.numpy()) and oob == int((~ok).any()) == int(c["name"].endswith("outside")), c["name"]


def test_loss_refs_against_torch():
    for c in G.loss_cases():
        lb = t(c["lb"]).double()
        want = -(lb.mean() + c["alpha"] * torch.tensor(c["log_qy"], dtype=torch.float64))
        loss, absum, nan = R.loss_fwd_ref(c["lb"], c["log_qy"], c["alpha"])
        assert nan == int(torch.isnan(lb).any() or c["poison"] == "inf") == int(c["poison"] is not None), c["name"]
        if not nan:
            assert abs(loss - float(want)) <= 1e-12 * abs(loss) and abs(absum - float(lb.abs().sum())) <= 1e-12 * absum
    for c in G.loss_bwd_cases():
        g = torch.tensor(1.0 if c["g"] is None else c["g"], dtype=torch.float32)
        d_lb, d_qy = R.loss_bwd_ref(float(g), c["alpha"], c["B"])
        assert eq_bits(d_lb, (-g / c["B"]).numpy()) and eq_bits(d_qy, (-torch.tensor(c["alpha"], dtype=torch.float32) * g).numpy())


def test_shard_refs_against_torch():
    for c in G.pack_cases():
        q, idx = t(c["q"]), t(c["idx"])
        want = torch.cat([q, idx.to(torch.int32).view(torch.float32)[:, None]], 1).view(torch.int32).numpy().view(np.uint32)
        words = R.shard_pack_ref(c["q"], c["idx"])
        assert np.array_equal(words, want), c["name"]
        pk = torch.from_numpy(words.view(np.int32).copy())
        uq, ui = R.shard_unpack_ref(words)
        assert np.array_equal(uq.view(np.uint32), pk[:, :-1].contiguous().numpy().view(np.uint32))
        assert np.array_equal(ui, pk[:, -1].to(torch.int64).numpy()) and np.array_equal(ui, c["idx"])
    assert {int(i) for c in G.pack_cases() for i in c["idx"]} >= set(G.PACK_IDX)
    for c in G.bwd_pack_cases():
        N, D, a, n = c["N"], c["D"], c["own0"], c["n_own"]
        left = t(c["dq_all"]) * torch.tensor(c["dq_scale"], dtype=torch.float32) if c["dq_all"] is not None else torch.zeros(N, D)
        right = torch.zeros(N, D)
        if c["dmu2_local"] is not None and n:
            right[a:a + n] = t(c["dmu2_local"])
        assert eq_bits(R.shard_bwd_pack_ref(c["dq_all"], c["dq_scale"], c["dmu2_local"], a, n, N, D), torch.cat([left, right], 1).numpy())
    for c in G.bwd_unpack_cases():
        buf, D, a, n = t(c["buf"]), c["D"], c["own0"], c["n_own"]
        dq, dm = R.shard_bwd_unpack_ref(c["buf"], a, n)
        assert eq_bits(dq, buf[a:a + n, :D].contiguous().numpy()) and eq_bits(dm, buf[:, D:].contiguous().numpy())


def test_sorted_run_lengths_sit_on_the_thresholds():
    L = list(G.sorted_run_lengths())
    at = int(np.cumsum(L)[L.index(257) - 1])
    assert at % 256 == 255 and L[1:] == G.SORTED_RUNS
    assert {63, 64, 65, 255, 256, 257, 31, 32, 33, 0, 600} <= set(L)


# ---------------------------------------------------------------------------------------------
# 2. the tables reject wrong kernels
# ---------------------------------------------------------------------------------------------
def rejected(cases, check, impl):
    """names of the cases on which `check(case, *impl(case))` fails; the oracle-built answer must pass on all of them"""
    bad = []
    for c in cases:
        try:
            check(c, *impl(c))
        except AssertionError:
            bad.append(c["name"])
    return bad


def _seg(c, zero_rows_normalised=False):
    btf, tbf, oob = R.segment_gather_ref(c["pool"], c["start"], c["T"], c["mean"], c["inv_std"])
    if zero_rows_normalised and c["mean"] is not None:
        fill = (F32(0) - c["mean"]) * c["inv_std"]
        for b, s in enumerate(c["start"]):
            for k in range(c["T"]):
                if not 0 <= s + k < c["pool"].shape[0]:
                    btf[b, k], tbf[k, b] = fill, fill
    return btf, tbf, oob


def test_wrong_segment_gather_is_rejected():
    cases = G.segment_gather_cases()
    assert not rejected(cases, G.check_segment_gather, _seg)
    bad = rejected(cases, G.check_segment_gather, lambda c: _seg(c, True))
    assert bad and all("mvn-all" in n for n in bad) and len(bad) == len(G.SEG_F)
    # a time-major output in batch-major order; a flag that is never raised; one raised by a legal last start
    assert rejected(cases, G.check_segment_gather, lambda c: (_seg(c)[0], _seg(c)[0].reshape(_seg(c)[1].shape), _seg(c)[2]))
    assert rejected(cases, G.check_segment_gather, lambda c: _seg(c)[:2] + (0,))
    assert rejected(cases, G.check_segment_gather, lambda c: _seg(c)[:2] + (int((c["start"] + c["T"] >= G.POOL_FRAMES).any()),))
    # fused (x - mean) * inv_std evaluated in higher precision and rounded once
    def once(c):
        if c["mean"] is None:
            return _seg(c)
        d = dict(c, pool=c["pool"].astype(np.float64), mean=c["mean"].astype(np.float64), inv_std=c["inv_std"].astype(np.float64))
        btf = np.zeros((len(c["start"]), c["T"], c["F"]))
        for b, s in enumerate(c["start"]):
            for k in range(c["T"]):
                if 0 <= s + k < G.POOL_FRAMES:
                    btf[b, k] = (d["pool"][s + k] - d["mean"]) * d["inv_std"]
        btf = btf.astype(F32)
        return btf, R.to_time_major_ref(btf), _seg(c)[2]
    assert rejected(cases, G.check_segment_gather, once)


def test_wrong_accumulate_and_finalize_are_rejected():
    cases = G.accumulate_cases()

    def right(c):
        zsum, _, cnt = R.mu2_accumulate_ref(c["z"], c["idx"], c["S"])
        return zsum.astype(F32), cnt.astype(F32)

    def counts_skipped(c):  # a skipped id is still counted: the rows with id S land in the last count
        zsum, cnt = right(c)
        cnt = cnt.copy()
        cnt[c["S"] - 1] += np.sum(c["idx"] == c["S"])
        return zsum, cnt

    def clamps(c):  # an id outside the range is clamped into it instead of skipped
        zsum, _, cnt = R.mu2_accumulate_ref(c["z"], np.clip(c["idx"], 0, c["S"] - 1), c["S"])
        return zsum.astype(F32), cnt.astype(F32)

    def bf16_sum(c):  # a sum that loses precision: rounded to bf16's 8 bits
        zsum, cnt = right(c)
        return (zsum.view(np.uint32) & 0xFFFF0000).view(F32), cnt

    assert not rejected(cases, G.check_accumulate, right)
    for wrong in (counts_skipped, clamps, bf16_sum):
        assert rejected(cases, G.check_accumulate, wrong), wrong.__name__
    fin = G.finalize_cases()
    assert not rejected(fin, G.check_finalize, lambda c: (R.mu2_finalize_ref(c["zsum"], c["cnt"], c["ratio"]),))
    with np.errstate(all="ignore"):
        assert rejected(fin, G.check_finalize, lambda c: (c["zsum"] / (c["cnt"][:, None] + F32(c["ratio"])),))  # no guard of count 0
        assert rejected(fin, G.check_finalize, lambda c: (R.mu2_finalize_ref(c["zsum"], c["cnt"], 0) if c["ratio"] < 1 else
                                                          R.mu2_finalize_ref(c["zsum"], c["cnt"], c["ratio"]),))  # ratio dropped
        rcp = lambda c: (np.where(c["cnt"][:, None] > 0, c["zsum"] * (F32(1) / (c["cnt"][:, None] + F32(c["ratio"]))), F32(0)).astype(F32),)
        assert rejected(fin, G.check_finalize, rcp)  # a reciprocal and a product instead of the division


def test_wrong_layout_kernels_are_rejected():
    cases = G.to_time_major_cases()

    def right(c):
        w = R.to_time_major_ref(c["x"])
        return w, R.bf16_rne(w), w

    def swapped(c):  # B and T exchanged in the split of the output index: b = (i / F) % T, t = i / (F T)
        B, T, F = c["x"].shape
        i = np.arange(B * T * F)
        f, b, t_ = i % F, (i // F) % T, i // (F * T)
        w = c["x"].ravel()[((b * T + t_) * F + f) % c["x"].size].reshape(T, B, F)  # (such a kernel reads past x: here it wraps)
        return w, R.bf16_rne(w), w

    assert not rejected(cases, G.check_to_time_major, right)
    bad = rejected(cases, G.check_to_time_major, swapped)
    assert len(bad) >= len(cases) - 1, bad  # every shape with B != T and more than one frame
    trunc = lambda x: (np.ascontiguousarray(x, F32).view(np.uint32) >> 16).astype(np.uint16)
    assert rejected(cases, G.check_to_time_major, lambda c: (right(c)[0], trunc(right(c)[0]), right(c)[2]))
    cast = G.cast_cases()
    assert not rejected(cast, G.check_cast, lambda c: (R.bf16_rne(c["x"]), np.ascontiguousarray(R.bf16_rne(c["x"]).T)))
    bad = rejected(cast, G.check_cast, lambda c: (trunc(c["x"]), None))
    assert len(bad) >= 4, bad
    # round half up instead of half to even: only the ties tell
    half_up = lambda x: ((np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64) + 0x8000) >> 16).astype(np.uint16)
    nan_safe = lambda x: np.where(np.isnan(x), np.uint16(0x7FC0), half_up(x))
    assert rejected(cast, G.check_cast, lambda c: (nan_safe(c["x"]), None))
    # a NaN that rounds into infinity (0x7F800001 + 0x7FFF carries nothing; truncated it is 0x7F80)
    assert rejected(cast, G.check_cast, lambda c: (np.where(np.isnan(c["x"]), trunc(c["x"]), R.bf16_rne(c["x"])), None))
    # the transposed destination written untransposed
    assert rejected(cast, G.check_cast, lambda c: (None, R.bf16_rne(c["x"]).reshape(c["x"].shape[1], c["x"].shape[0])))
    # denormals flushed to zero
    den = [G.cast_denormal_case()]
    assert not rejected(den, G.check_cast, lambda c: (R.bf16_rne(c["x"]), None))
    assert rejected(den, G.check_cast, lambda c: (R.bf16_rne(np.where(np.abs(c["x"]) < 2.0 ** -126, np.copysign(F32(0), c["x"]), c["x"])), None))


def test_wrong_gather_is_rejected():
    cases = G.gather_cases()
    assert not rejected(cases, G.check_gather, lambda c: R.gather_fwd_ref(c["table"], c["idx"], c["off"]))
    bad = rejected(cases, G.check_gather, lambda c: R.gather_fwd_ref(c["table"], c["idx"], 0))  # without idx_offset
    assert bad and all("off6" in n for n in bad)
    assert rejected(cases, G.check_gather, lambda c: (R.gather_fwd_ref(c["table"], c["idx"], c["off"])[0], 0))

    def clamped(c):  # a row outside the shard read from its nearest row
        S = c["table"].shape[0]
        return c["table"][np.clip(c["idx"] - c["off"], 0, S - 1)], R.gather_fwd_ref(c["table"], c["idx"], c["off"])[1]
    assert rejected(cases, G.check_gather, clamped)
    i32 = lambda c: R.gather_fwd_ref(c["table"], c["idx"].astype(np.int32).astype(np.int64), c["off"])  # idx cut to 32 bits
    assert rejected(cases, G.check_gather, i32)


def test_wrong_loss_is_rejected():
    cases = G.loss_cases()

    def mean64(lb, B):
        with np.errstate(invalid="ignore"):
            return lb.astype(np.float64).sum() / B

    def f32_loss(lb, c):
        m = mean64(lb, c["B"])
        return F32(-(m + c["alpha"] * c["log_qy"])), int(np.isnan(m))

    assert not rejected(cases, G.check_loss_fwd, lambda c: f32_loss(c["lb"], c))
    drop = lambda c: f32_loss(c["lb"][:c["B"] // 256 * 256], c)  # the last partial stride of 256 is not summed
    bad = rejected(cases, G.check_loss_fwd, drop)
    assert {n.split("-")[0] for n in bad} == {"B%d" % b for b in G.LOSS_B if b % 256}, bad
    assert rejected(cases, G.check_loss_fwd, lambda c: (f32_loss(c["lb"], c)[0], 0))           # the word is never raised
    assert rejected(cases, G.check_loss_fwd, lambda c: (f32_loss(c["lb"], c)[0], int(np.isnan(c["lb"][0]))))  # only element 0 looked at
    assert rejected(cases, G.check_loss_fwd, lambda c: (F32(-mean64(c["lb"], c["B"])), f32_loss(c["lb"], c)[1]))  # alpha dropped
    assert rejected(cases, G.check_loss_fwd, lambda c: (F32(float(f32_loss(c["lb"], c)[0]) * (1 + 2.0 ** -17)), f32_loss(c["lb"], c)[1]))  # seven bits short
    bwd = G.loss_bwd_cases()
    right = lambda c: (np.full(c["B"], R.loss_bwd_ref(c["g"] or 1.0, c["alpha"], c["B"])[0]), np.asarray([R.loss_bwd_ref(c["g"] or 1.0, c["alpha"], c["B"])[1]]))
    assert not rejected(bwd, G.check_loss_bwd, right)
    assert rejected(bwd, G.check_loss_bwd, lambda c: (np.full(c["B"], F32(-(c["g"] or 1.0)) * (F32(1) / F32(c["B"]))), None))  # reciprocal
    assert rejected(bwd, G.check_loss_bwd, lambda c: (np.full(c["B"], R.loss_bwd_ref(1.0, c["alpha"], c["B"])[0]), None))       # g ignored


def test_wrong_shard_helpers_are_rejected():
    cases = G.pack_cases()
    assert not rejected(cases, G.check_pack, lambda c: (R.shard_pack_ref(c["q"], c["idx"]),))
    by_value = lambda c: (np.concatenate([c["q"], c["idx"].astype(F32)[:, None]], 1).view(np.uint32),)  # value cast of the index
    assert len(rejected(cases, G.check_pack, by_value)) == len(cases)
    assert not rejected(cases, G.check_unpack, lambda c: R.shard_unpack_ref(R.shard_pack_ref(c["q"], c["idx"])))

    def unpack_by_value(c):
        w = R.shard_pack_ref(c["q"], c["idx"])
        with np.errstate(invalid="ignore"):
            return w[:, :-1].copy().view(F32), np.nan_to_num(w[:, -1].copy().view(F32)).astype(np.int64)
    assert len(rejected(cases, G.check_unpack, unpack_by_value)) == len(cases)
    # a matched pair of value casts survives every round trip below 2^24 and is wrong above: the tables hold 2^24 + 1
    for c in cases:
        assert not np.array_equal(c["idx"].astype(F32).astype(np.int64), c["idx"]), c["name"]

    pk = G.bwd_pack_cases()
    ref = lambda c, **kw: (R.shard_bwd_pack_ref(*[kw.get(k, c[k]) for k in ("dq_all", "dq_scale", "dmu2_local", "own0", "n_own", "N", "D")]),)
    assert not rejected(pk, G.check_bwd_pack, ref)

    def shifted(c):  # the own range one row late
        out = R.shard_bwd_pack_ref(c["dq_all"], c["dq_scale"], None, 0, 0, c["N"], c["D"])
        if c["dmu2_local"] is not None:
            for j in range(c["n_own"]):
                if c["own0"] + 1 + j < c["N"]:
                    out[c["own0"] + 1 + j, c["D"]:] = c["dmu2_local"][j]
        return (out,)
    bad = rejected(pk, G.check_bwd_pack, shifted)
    assert bad and {n.split("-")[0] for n in bad} == {"N%d" % n for n, _ in G.BWD_SHAPES}
    assert rejected(pk, G.check_bwd_pack, lambda c: ref(c, dq_scale=1.0))      # the scale dropped
    assert rejected(pk, G.check_bwd_pack, lambda c: ref(c, own0=0))            # the own range always at row 0
    un = G.bwd_unpack_cases()
    assert not rejected(un, G.check_bwd_unpack, lambda c: R.shard_bwd_unpack_ref(c["buf"], c["own0"], c["n_own"]))
    assert rejected(un, G.check_bwd_unpack, lambda c: R.shard_bwd_unpack_ref(c["buf"], 0, c["n_own"]))   # dq of the first rows
    halves = lambda c: (R.shard_bwd_unpack_ref(c["buf"], c["own0"], c["n_own"])[0], c["buf"][:, :c["D"]])  # dmu2 from the dq half
    assert rejected(un, G.check_bwd_unpack, halves)


# ---------------------------------------------------------------------------------------------
# 3. argument errors: returned on the host, before any launch
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding as hb

    return hb.load_library()


def _codes(lib):
    text = open(os.path.join(ROOT, "include", "fhvae_hip.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"\b(FHVAE_(?:OK|ERR_[A-Z]+))\s*=\s*(-?\d+)", text)}
    assert len(codes) == 6
    for name, word in (("NULL", b"NULL"), ("SHAPE", b"dimension"), ("DTYPE", b"dtype"), ("ALIGN", b"aligned"), ("LIMIT", b"index range")):
        assert word in lib.fhvae_strerror(codes["FHVAE_ERR_" + name])
    return codes


def test_glue_argument_errors_are_reported_before_any_launch(lib):
    E = _codes(lib)
    OK, NULL, SHAPE, DTYPE, LIMIT = E["FHVAE_OK"], E["FHVAE_ERR_NULL"], E["FHVAE_ERR_SHAPE"], E["FHVAE_ERR_DTYPE"], E["FHVAE_ERR_LIMIT"]
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # segment_gather: no output at all; mean without inv_std and the reverse
    assert lib.fhvae_segment_gather(p, 50, p, None, None, None, None, 2, 5, 8, None, None) == NULL
    assert lib.fhvae_segment_gather(p, 50, p, p, None, p, p, 2, 5, 8, None, None) == NULL
    assert lib.fhvae_segment_gather(p, 50, p, None, p, p, None, 2, 5, 8, None, None) == NULL
    assert lib.fhvae_segment_gather(p, 0, p, None, None, p, None, 2, 5, 8, None, None) == SHAPE
    assert lib.fhvae_cast_bf16(p, None, None, 4, 4, None) == NULL
    assert lib.fhvae_cast_bf16(None, p, p, 4, 4, None) == NULL
    import hip_binding as hb

    assert lib.fhvae_to_time_major(p, p, None, 2, 3, 4, max(hb.F32, hb.BF16) + 1, None) == DTYPE
    assert lib.fhvae_to_time_major(p, p, p, 2, 3, 10, -1, None) == DTYPE
    assert lib.fhvae_to_time_major(p, None, p, 2, 3, 4, hb.F32, None) == NULL
    assert lib.fhvae_mu2_accumulate_sorted(p, p, p, p, 10, 4, 257, p, None) == LIMIT
    assert lib.fhvae_mu2_accumulate_sorted(p, p, p, p, 10, 4, 256, None, None) == NULL
    K = 4
    assert lib.fhvae_mu2_merge_load_shard(p, 1, K, 3, 2, p, p, p, 2, 0.25, None) == SHAPE   # row1 < row0
    assert lib.fhvae_mu2_merge_load_shard(p, 1, K, -1, 2, p, p, p, 2, 0.25, None) == SHAPE  # row0 < 0
    assert lib.fhvae_mu2_merge_load_shard(p, 1, K, 0, K + 1, p, p, p, 2, 0.25, None) == SHAPE  # row1 > K
    assert lib.fhvae_mu2_merge_load_shard(p, 1, K, 2, 2, None, None, None, 2, 0.25, None) == OK  # an empty shard: nothing to load
    assert lib.fhvae_mu2_merge_load_shard(p, 1, K, K, K, None, None, None, 2, 0.25, None) == OK
    assert lib.fhvae_loss_fwd(p, p, 10.0, p, 2 ** 31, None, None) == LIMIT
    assert lib.fhvae_loss_fwd(p, p, 10.0, p, 0, None, None) == SHAPE
    assert lib.fhvae_loss_fwd(p, None, 10.0, p, 8, None, None) == NULL
    assert lib.fhvae_loss_bwd(None, 10.0, None, None, 8, None) == NULL
    assert lib.fhvae_hs_select(p, 10, p, 4, p, p, p, -1, p, None) == SHAPE                  # cap < 0
    assert lib.fhvae_hs_select(p, 10, p, 4, None, p, p, 1, p, None) == NULL                 # cap > 0 without seg_ids
    assert lib.fhvae_hs_select(p, 10, p, 4, p, None, p, 1, p, None) == NULL                 # ... without local_idx
    assert lib.fhvae_hs_select(p, 10, p, 4, p, p, p, 1, None, None) == NULL                 # no status word
    for fn in (lib.fhvae_shard_pack, lib.fhvae_shard_unpack):
        assert fn(p, p, None, 4, 4, None) == NULL and fn(p, p, p, 0, 4, None) == SHAPE
    assert lib.fhvae_shard_bwd_pack(None, 1.0, None, 0, 0, None, 4, 4, None) == NULL
    assert lib.fhvae_shard_bwd_unpack(None, 0, 0, None, None, 4, 4, None) == NULL
