"""The case tables and comparators of the data / layout / exchange kernels, shared by tests/test_glue_gpu.py (which runs the
kernels on them) and tests/test_glue_cpu.py (which checks the oracles of tests/glue_ref.py on them against torch-CPU
expressions, and that plausible wrong kernels are rejected by them).  numpy only.

A comparator takes a case and what an implementation returned for it (numpy arrays) and raises AssertionError.  The three
summed quantities return the share of their bound that was taken."""
import itertools

import numpy as np

import glue_ref as R

F32 = np.float32
U = 2.0 ** -24  # unit roundoff of float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: got %r want %r" % (
        what, bad.size, want.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


# ---------------------------------------------------------------------------------------------
# segment_gather: a pool of 50 frames, T = 5
# ---------------------------------------------------------------------------------------------
POOL_FRAMES, SEG_T = 50, 5
SEG_F = (8, 80, 3, 10)  # V = 4: 8, 80; V = 1: 3, 10
_P, _T = POOL_FRAMES, SEG_T
SEG_STARTS = {
    "inside": [17, 3, 17, 0, _P - _T, 31],                                       # interior (one repeated), both last legal starts
    "all": [17, 0, _P - _T, -2, _P - _T + 2, -_T - 1, _P + 3, 3, -_T, _P, _P - 1, 1 - _T],  # + straddling either end, wholly outside
}


def segment_gather_cases():
    out = []
    for F, mvn, starts in itertools.product(SEG_F, (False, True), SEG_STARTS):
        rng = np.random.default_rng(1000 + F)
        c = {"name": "F%d-%s-%s" % (F, "mvn" if mvn else "raw", starts), "F": F, "T": SEG_T,
             "pool": (rng.standard_normal((POOL_FRAMES, F)) * 3 + 2).astype(F32), "start": np.asarray(SEG_STARTS[starts], np.int64),
             "mean": None, "inv_std": None}
        if mvn:
            c["mean"] = (rng.standard_normal(F) + 2).astype(F32)
            c["inv_std"] = (1 / rng.uniform(0.5, 3, F)).astype(F32)
        out.append(c)
    return out


def check_segment_gather(c, btf, tbf, flag):
    """btf / tbf: None where the output was not requested; flag: None when no flag word was passed."""
    w_btf, w_tbf, w_oob = R.segment_gather_ref(c["pool"], c["start"], c["T"], c["mean"], c["inv_std"])
    if btf is not None:
        same_bits(btf, w_btf, c["name"] + " batch-major")
    if tbf is not None:
        same_bits(tbf, w_tbf, c["name"] + " time-major")
    if flag is not None:
        assert int(flag) == w_oob, (c["name"], "oob flag", int(flag), w_oob)


# ---------------------------------------------------------------------------------------------
# mu2_accumulate / mu2_finalize
# ---------------------------------------------------------------------------------------------
ACC_SHAPES = ((1, 1, 1), (257, 5, 3), (1000, 37, 16), (600, 4, 32))
FIN_RATIOS = (0.25, 0.0, 1e3)


def accumulate_cases():
    out = []
    for N, S, D in ACC_SHAPES:
        rng = np.random.default_rng(N + S + D)
        z = (rng.standard_normal((N, D)) * 3 + 1).astype(F32)
        if N == 1:
            idx = np.zeros(1, np.int64)
        else:
            live = np.arange(S) if S <= 5 else np.setdiff1d(np.arange(S), [2, S - 1, S // 2])  # S > 5: three ids never occur
            if (N, S) == (257, 5):
                live = np.array([0, 1, 4])  # ids 2 and 3 never occur
            idx = rng.choice(live, size=N).astype(np.int64)
            idx[[1, N // 2, N - 1]] = -1
            idx[[0, N // 3, N - 2]] = S
            idx[5] = -(2 ** 40)
            idx[6] = 2 ** 40 + 1
        out.append({"name": "N%d-S%d-D%d" % (N, S, D), "N": N, "S": S, "D": D, "z": z, "idx": idx})
    return out


def check_accumulate(c, zsum, cnt):
    """counts exact; per element |zsum - sum64| <= n_s 2^-24 sum|z| (n_s the id's row count): the first-order bound of n_s float
    additions in ANY order is (n_s - 1) u sum|z|; n_s covers the higher-order terms.  Returns the worst share."""
    want, absum, n = R.mu2_accumulate_ref(c["z"], c["idx"], c["S"])
    assert np.array_equal(np.asarray(cnt, np.float64), n.astype(np.float64)), (c["name"], "counts", cnt, n)
    err = np.abs(np.asarray(zsum, np.float64) - want)
    bound = n[:, None] * U * absum
    assert (err <= bound).all(), (c["name"], "sum", float((err / np.maximum(bound, 1e-300)).max()))
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def finalize_cases():
    out = []
    for (N, S, D), ratio in itertools.product(ACC_SHAPES, FIN_RATIOS):
        rng = np.random.default_rng(S * 100 + D)
        zsum = (rng.standard_normal((S, D)) * 40).astype(F32)  # rows with count 0 keep a non-zero sum: they must still give 0
        cnt = rng.integers(1, 200, size=S).astype(F32)
        cnt[::3] = 0
        if S == 1:
            cnt[0] = 7 if ratio else 0
        out.append({"name": "S%d-D%d-r%g" % (S, D, ratio), "S": S, "D": D, "zsum": zsum, "cnt": cnt, "ratio": ratio})
    return out


def check_finalize(c, mu2):
    same_bits(mu2, R.mu2_finalize_ref(c["zsum"], c["cnt"], c["ratio"]), c["name"])


# ---------------------------------------------------------------------------------------------
# to_time_major / cast_bf16
# ---------------------------------------------------------------------------------------------
TTM_SHAPES = ((1, 1, 4), (3, 2, 4), (7, 3, 10), (5, 4, 12), (65, 3, 80), (2, 257, 8))


def to_time_major_cases():
    out = []
    for B, T, F in TTM_SHAPES:
        rng = np.random.default_rng(B * 1000 + T * 10 + F)
        out.append({"name": "B%d-T%d-F%d" % (B, T, F), "x": (rng.standard_normal((B, T, F)) * 2).astype(F32)})
    return out


def same_bf16(got, want, what):
    got, want = np.asarray(got, np.uint16), np.asarray(want, np.uint16)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = R.bf16_is_nan(want)
    assert np.array_equal(R.bf16_is_nan(got), nan), (what, "NaN positions")
    bad = np.flatnonzero((got != want).ravel() & ~nan.ravel())
    assert bad.size == 0, "%s: %d of %d bf16 words differ, first at %d: got 0x%04x want 0x%04x" % (
        what, bad.size, want.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def check_to_time_major(c, out_f32=None, out_bf16=None, out_copy=None):
    want = R.to_time_major_ref(c["x"])
    if out_f32 is not None:
        same_bits(out_f32, want, c["name"] + " f32")
    if out_bf16 is not None:
        same_bf16(out_bf16, R.bf16_rne(want), c["name"] + " bf16")
    if out_copy is not None:
        same_bits(out_copy, want, c["name"] + " x_tbf_f32")


CAST_SHAPES = ((1, 1), (1, 37), (37, 1), (33, 65), (64, 64))
#: the edge values, at flat positions 0, 1, ... of the input (as many as the shape holds)
CAST_EDGE_BITS = np.array([
    0x00000000, 0x80000000,    # +0, -0
    0x3F808000,                # 1 + 2^-8: a tie, to even = down (0x3F80)
    0x3F818000,                # 1 + 3 2^-8: a tie, to even = up (0x3F82)
    0x3F808001,                # 1 + 2^-8 + 2^-23: above the tie, up (0x3F81)
    0x7F7F7FFF,                # the largest value that still rounds to the largest finite bf16 (0x7F7F)
    0x7F7F8000,                # a tie that rounds to +inf (0x7F80)
    0x7F800000, 0xFF800000,    # +inf, -inf
    0x7FC00001, 0x7F800001,    # a quiet and a signalling NaN
    0xFFC00000, 0xFF7F8000,    # a negative NaN; the negative tie that rounds to -inf
    0xBF818000,                # -(1 + 3 2^-8)
], np.uint32)
CAST_DENORMAL_BITS = np.array([0x00008000, 0x00018000, 0x00000001, 0x00007FFF, 0x00008001, 0x007FFFFF, 0x007F8000, 0x80008000,
                               0x80018000, 0x00010000, 0x00400000, 0x807FFFFF], np.uint32)


def cast_cases():
    out = []
    for R_, C_ in CAST_SHAPES:
        rng = np.random.default_rng(R_ * 100 + C_)
        x = (rng.standard_normal(R_ * C_) * np.exp(rng.uniform(-20, 20, R_ * C_))).astype(F32)
        k = min(x.size, CAST_EDGE_BITS.size)
        x.view(np.uint32)[:k] = CAST_EDGE_BITS[:k]
        out.append({"name": "R%d-C%d" % (R_, C_), "x": x.reshape(R_, C_)})
    return out


def cast_denormal_case():
    """f32 denormals in a (3, 4) matrix.  oracle/lstm_lp_ref.py's rb() (torch's float -> bfloat16) rounds them like any other
    value, which is what bf16_rne does: a kernel that flushes them to zero differs here."""
    return {"name": "denormals", "x": CAST_DENORMAL_BITS.view(F32).reshape(3, 4).copy()}


def check_cast(c, dst=None, dst_t=None):
    want = R.bf16_rne(c["x"])
    if dst is not None:
        same_bf16(dst, want, c["name"] + " dst")
    if dst_t is not None:
        same_bf16(dst_t, np.ascontiguousarray(want.T), c["name"] + " dst_t")


# ---------------------------------------------------------------------------------------------
# mu2_gather_fwd
# ---------------------------------------------------------------------------------------------
GATHER_SHAPES = ((1, 1, 1), (9, 6, 4), (300, 50, 32))
GATHER_OFFS = (0, 6)


def gather_cases():
    out = []
    for (B, S, D), off, outside in itertools.product(GATHER_SHAPES, GATHER_OFFS, (False, True)):
        rng = np.random.default_rng(B + S + D + off)
        table = rng.standard_normal((S, D)).astype(F32)
        idx = (rng.integers(0, S, size=B) + off).astype(np.int64)
        if B == 1:
            idx[0] = off + S if outside else off
        else:
            idx[[0, 1, 2, 3]] = [off, off + S - 1, off + S - 1, off]  # both ends of the shard, repeated
            if outside:
                idx[[4, 5, 6, 7, 8]] = [off - 1, off + S, -3, off - 2 ** 33, off + 2 ** 33 + 1]
        out.append({"name": "B%d-S%d-D%d-off%d-%s" % (B, S, D, off, "outside" if outside else "inside"), "table": table,
                    "idx": idx, "off": off})
    return out


def check_gather(c, out, flag):
    want, oob = R.gather_fwd_ref(c["table"], c["idx"], c["off"])
    same_bits(out, want, c["name"])
    if flag is not None:
        assert int(flag) == oob, (c["name"], "oob flag", int(flag), oob)


# ---------------------------------------------------------------------------------------------
# loss_fwd / loss_bwd
# ---------------------------------------------------------------------------------------------
LOSS_B = (1, 63, 64, 255, 256, 257, 511, 4099)
LOSS_ALPHA = (0.0, 10.0)
LOSS_LOG_QY = -7.25


def loss_cases():
    """poison: None, ("nan", position) or "inf" (+inf and -inf in one batch: their sum is NaN)."""
    out = []
    for B, alpha in itertools.product(LOSS_B, LOSS_ALPHA):
        rng = np.random.default_rng(B)
        lb = (rng.standard_normal(B) * 30 - 100).astype(F32)
        poisons = [None]
        if alpha:
            poisons += [("nan", p) for p in sorted({0, 255, 256, B - 1}) if p < B] + (["inf"] if B > 1 else [])
        for p in poisons:
            x = lb.copy()
            if p == "inf":
                x[0], x[B - 1] = np.inf, -np.inf
            elif p:
                x[p[1]] = np.nan
            out.append({"name": "B%d-a%g-%s" % (B, alpha, "clean" if p is None else p if p == "inf" else "nan%d" % p[1]),
                        "B": B, "alpha": alpha, "lb": x, "log_qy": LOSS_LOG_QY, "poison": p})
    return out


def loss_bound(B, absum, alpha, log_qy):
    """(ceil(B/256) + 12) 2^-24 (sum|lb| / B + |alpha log_qy|): see the docstring of tests/test_glue_gpu.py."""
    return (-(-B // 256) + 12) * U * (absum / B + abs(alpha * log_qy))


def check_loss_fwd(c, loss, flag):
    want, absum, nan = R.loss_fwd_ref(c["lb"], c["log_qy"], c["alpha"])
    if flag is not None:
        assert int(flag) == nan, (c["name"], "nan flag", int(flag), nan)
    if nan:
        assert np.isnan(loss), (c["name"], loss)
        return 0.0
    bound = loss_bound(c["B"], absum, c["alpha"], c["log_qy"])
    err = abs(float(loss) - want)
    assert err <= bound, (c["name"], float(loss), want, err / bound)
    return err / bound


def loss_bwd_cases():
    return [{"name": "B%d-a%g-g%s" % (B, alpha, g), "B": B, "alpha": alpha, "g": g}
            for B, alpha, g in itertools.product(LOSS_B, LOSS_ALPHA, (None, 0.37))]


def check_loss_bwd(c, d_lb, d_qy):
    w_lb, w_qy = R.loss_bwd_ref(1.0 if c["g"] is None else c["g"], c["alpha"], c["B"])
    same_bits(d_lb, np.full(c["B"], w_lb, F32), c["name"] + " d_lower_bound")
    if d_qy is not None:
        same_bits(d_qy, np.asarray([w_qy], F32), c["name"] + " d_log_qy")


# ---------------------------------------------------------------------------------------------
# the row shard's exchange helpers
# ---------------------------------------------------------------------------------------------
PACK_SHAPES = ((1, 1), (5, 3), (300, 32))
#: as floats these words are a zero, denormals, an ordinary value and NaNs
PACK_IDX = (0, 1, 2 ** 23 - 1, 2 ** 24 + 1, 2 ** 30 + 3, 2 ** 31 - 1)


def pack_cases():
    out = []
    for B, D in PACK_SHAPES:
        rng = np.random.default_rng(B * 7 + D)
        idx = rng.integers(0, 2 ** 31, size=B).astype(np.int64)
        head = [2 ** 24 + 1] if B == 1 else list(PACK_IDX)[-B:] if B < len(PACK_IDX) else list(PACK_IDX)
        idx[:len(head)] = head
        q = rng.standard_normal((B, D)).astype(F32)
        out.append({"name": "B%d-D%d" % (B, D), "q": q, "idx": idx})
    return out


def check_pack(c, words):
    want = R.shard_pack_ref(c["q"], c["idx"])
    got = np.asarray(words, np.uint32)
    assert got.shape == want.shape and np.array_equal(got, want), (c["name"], np.flatnonzero((got != want).ravel())[:4])


def check_unpack(c, q, idx):
    """the input of unpack is shard_pack_ref(c), built by the oracle."""
    w_q, w_idx = R.shard_unpack_ref(R.shard_pack_ref(c["q"], c["idx"]))
    same_bits(q, w_q, c["name"] + " q")
    idx = np.asarray(idx)
    assert idx.dtype == np.int64 and np.array_equal(idx, w_idx), (c["name"], "idx", idx[:8], w_idx[:8])


BWD_SHAPES = ((1, 1), (10, 3), (300, 32))
BWD_DQ = (None, 1.0, 0.5, -3.0)  # None: dq_all NULL


def own_ranges(N):
    """(own0, n_own): the whole buffer, its first rows, its last rows, an empty range -- cut to the N rows there are."""
    k = min(3, N)
    return sorted({(0, N), (0, k), (N - k, k), (4, 0)})


def bwd_pack_cases():
    out = []
    for N, D in BWD_SHAPES:
        rng = np.random.default_rng(N * 3 + D)
        dq, dmu2 = rng.standard_normal((N, D)).astype(F32), rng.standard_normal((N, D)).astype(F32)
        for (own0, n_own), scale, with_dmu2 in itertools.product(own_ranges(N), BWD_DQ, (False, True)):
            out.append({"name": "N%d-D%d-own%d+%d-dq%s-dmu2%d" % (N, D, own0, n_own, scale, with_dmu2), "N": N, "D": D,
                        "own0": own0, "n_own": n_own, "dq_all": None if scale is None else dq, "dq_scale": 1.0 if scale is None else scale,
                        "dmu2_local": dmu2[:n_own] + 5 if with_dmu2 else None})
    return out


def check_bwd_pack(c, out):
    same_bits(out, R.shard_bwd_pack_ref(c["dq_all"], c["dq_scale"], c["dmu2_local"], c["own0"], c["n_own"], c["N"], c["D"]), c["name"])


def bwd_unpack_cases():
    out = []
    for N, D in BWD_SHAPES:
        rng = np.random.default_rng(N * 5 + D)
        buf = rng.standard_normal((N, 2 * D)).astype(F32)
        for (own0, n_own), (want_dq, want_dmu2) in itertools.product(own_ranges(N), ((True, True), (False, True), (True, False))):
            out.append({"name": "N%d-D%d-own%d+%d-dq%d-dmu2%d" % (N, D, own0, n_own, want_dq, want_dmu2), "N": N, "D": D, "buf": buf,
                        "own0": own0, "n_own": n_own, "want_dq": want_dq, "want_dmu2": want_dmu2})
    return out


def check_bwd_unpack(c, dq_local, dmu2_all):
    w_dq, w_dm = R.shard_bwd_unpack_ref(c["buf"], c["own0"], c["n_own"])
    if dq_local is not None:
        same_bits(dq_local, w_dq, c["name"] + " dq_local")
    if dmu2_all is not None:
        same_bits(dmu2_all, w_dm, c["name"] + " dmu2_all")


# ---------------------------------------------------------------------------------------------
# mu2_accumulate_sorted (csrc/hs.hip): run lengths on its thresholds, for tests/test_hs_gpu.py
# ---------------------------------------------------------------------------------------------
SORTED_D = (24, 48, 100, 200, 256)
SORTED_RUNS = [1, 63, 64, 65, 0, 255, 256, 257, 31, 32, 33, 1, 600, 2]


def sorted_run_lengths():
    """SORTED_RUNS behind a filler run that puts the first row of the 257-run on the last row a workgroup owns (row index = 255
    mod 256)."""
    before = sum(SORTED_RUNS[:SORTED_RUNS.index(257)])
    filler = (255 - before) % 256
    lengths = [filler] + SORTED_RUNS
    assert filler > 0 and sum(lengths[:lengths.index(257)]) % 256 == 255
    return np.asarray(lengths, np.int64)
