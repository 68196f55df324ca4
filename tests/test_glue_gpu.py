"""The kernels that move data around the training step's compute kernels, on a MI355X, each against its numpy oracle
(tests/glue_ref.py) on the case tables of tests/glue_cases.py: fhvae_segment_gather, fhvae_mu2_accumulate / _finalize
(csrc/data.hip); fhvae_to_time_major, fhvae_cast_bf16, fhvae_mu2_gather_fwd, fhvae_loss_fwd / _bwd and the four fhvae_shard_*
helpers (csrc/loss.hip).  tests/test_glue_cpu.py checks the oracles and that the tables reject wrong kernels.

The entry points are called directly (hb._call with raw pointers), so NULL operands, flag words and misaligned views are
reached.  Every case keeps the buffer discipline of tests/test_gemm_oracle_gpu.py: an output is a sub-range of a larger buffer
of a sentinel that must come back untouched, and starts as NaN (float) or a marker (integers), so an element that was never
written shows; an input is the leading part of an allocation whose remainder is NaN (float) or far outside every range
(indices); a flag word sits between two sentinel words and is checked both ways -- raised when it must be, still 0 when not.
Only inputs the kernels guard are given (data.hip:26, :56; loss.hip:65): a frame outside the pool, an id outside the table.
A misaligned view starts inside an allocation that holds the whole view.  Nothing here has 2^31 elements: the 64-bit index
paths of these kernels stay unpinned.

Bit-exact: every copy, the bf16 conversion (NaNs compare as NaN, not by payload), the normalisation (x - mean) * inv_std (a
difference and a product cannot be contracted: two float32 roundings, as numpy's), mu2_finalize's zsum / (count + ratio),
loss_bwd's -g / B and -alpha * g.

Bounds of the three summed quantities (u = 2^-24):
  * mu2_accumulate: |zsum - sum64| <= n_s u sum|z| per element, n_s the id's row count.  The float atomics add the n_s
    values in some order; for ANY order the first-order error of n_s - 1 additions is (n_s - 1) u sum|z|, and the factor n_s
    covers the higher-order terms.  Two calls over a split keep the bound (the same n_s additions in another order).
  * mu2_accumulate_sorted at D in {24, 48, 100, 200, 256} (tests/test_hs_gpu.py): the bound of its existing test,
    (n_s + 2) u sum|z| -- serial chains of at most n_s rows; pieces and the group sums only shorten them.
  * loss_fwd: |loss - loss64| <= (ceil(B/256) + 12) u (sum|lb| / B + |alpha log_qy|).  From loss.hip's loss_fwd_kernel: a thread
    adds at most ceil(B/256) terms to 0 (the first addition is exact), wave_sum is 6 butterfly additions, thread 0 adds the 4
    wave sums with 3 additions: every partial sum is bounded by sum|lb|, so the sum carries at most (ceil(B/256) + 9) u sum|lb|;
    the division by B adds one rounding, u sum|lb| / B; alpha * log_qy and the addition to the mean are two roundings (one if
    contracted to an fma), at most u |alpha log_qy| + u (sum|lb| / B + |alpha log_qy|); the negation is exact.  Together
    (ceil(B/256) + 11) u sum|lb| / B + 2 u |alpha log_qy|, inside the bound; the twelfth unit covers the higher-order terms.

Measured on an MI355X (worst share of the bound taken, per entry; printed by the tests):
  mu2_accumulate (N, S, D)      (1, 1, 1) 0.000   (257, 5, 3) 0.032   (1000, 37, 16) 0.136   (600, 4, 32) 0.034
  mu2_accumulate_sorted D       24: 0.220   48: 0.217   100: 0.237   200: 0.240   256: 0.250
  loss_fwd B                    1: 0.000   63: 0.144   64: 0.009   255: 0.111   256: 0.038   257: 0.054   511: 0.015   4099: 0.035
Every bit-exact assertion holds as written, the f32 denormals of test_cast_bf16_denormals included; no sentinel touched.
"""
import numpy as np
import pytest
import torch

import glue_cases as G
import glue_ref as R

pytestmark = pytest.mark.gpu

from test_ops_gpu import hb  # noqa: F401,E402

NAN = float("nan")
#: per dtype: (sentinel around a buffer, what an output holds before the launch, what follows an input)
FILL = {torch.float32: (-12345.0, NAN, NAN), torch.int16: (0x5A5A, 0x5555, 0x7FC1), torch.int64: (-7, -9, 1 << 62),
        torch.int32: (77, 0, 77)}
LEAD = 16  # elements in front of every view: 64 bytes of f32, 32 of bf16 -- a view with mis = 0 is 16-byte aligned


class Out:
    """n elements at LEAD + mis of a buffer of sentinels; mis = 1 puts the view one element (4 bytes of f32, 2 of bf16) past
    a 16-byte boundary."""

    def __init__(self, n, dtype=torch.float32, mis=0, start=None):
        sent, first, _ = FILL[dtype]
        self.full = torch.full((LEAD + mis + n + LEAD,), sent, dtype=dtype, device="cuda")
        self.lo, self.n, self.sent = LEAD + mis, n, sent
        self.full[self.lo:self.lo + n] = first if start is None else start
        self.ptr = self.full.data_ptr() + self.lo * self.full.element_size()
        assert (self.ptr % 16 == 0) == (mis == 0)

    def get(self, *shape):
        """the view as numpy, after checking that nothing around it was written"""
        h = self.full.cpu().numpy()
        around = np.concatenate([h[:self.lo], h[self.lo + self.n:]])
        assert (around == np.asarray(self.sent, h.dtype)).all(), "written outside the output: %r" % (np.flatnonzero(around != self.sent)[:8],)
        v = h[self.lo:self.lo + self.n]
        return v.reshape(shape) if shape else v


class In:
    """a numpy array as the leading part (from LEAD + mis) of a larger allocation"""

    def __init__(self, a, mis=0):
        a = np.ascontiguousarray(a)
        dtype = torch.from_numpy(a[:0].copy()).dtype
        self.full = torch.full((LEAD + mis + a.size + LEAD,), FILL[dtype][2], dtype=dtype, device="cuda")
        self.full[LEAD + mis:LEAD + mis + a.size] = torch.from_numpy(a.ravel()).cuda()
        self.ptr = self.full.data_ptr() + (LEAD + mis) * self.full.element_size()


def ptr(x):
    return None if x is None else x.ptr


class Flag(Out):
    """an int32 device word, 0, between sentinel words"""

    def __init__(self):
        super().__init__(1, torch.int32)

    def value(self):
        return int(self.get()[0])


def u16(a):
    return a.view(np.uint16)


# ---------------------------------------------------------------------------------------------
# segment_gather
# ---------------------------------------------------------------------------------------------
def run_seg(hb, c, outs=("btf", "tbf"), flag=True, mis=(0, 0, 0)):
    B, T, F = len(c["start"]), c["T"], c["F"]
    pool, start = In(c["pool"], mis[0]), In(c["start"])
    mean = In(c["mean"]) if c["mean"] is not None else None
    inv_std = In(c["inv_std"]) if c["inv_std"] is not None else None
    btf = Out(B * T * F, mis=mis[1]) if "btf" in outs else None
    tbf = Out(B * T * F, mis=mis[2]) if "tbf" in outs else None
    fl = Flag() if flag else None
    hb._call("fhvae_segment_gather", pool.ptr, c["pool"].shape[0], start.ptr, ptr(mean), ptr(inv_std), ptr(btf), ptr(tbf), B, T, F,
             ptr(fl))
    got = (btf.get(B, T, F) if btf else None, tbf.get(T, B, F) if tbf else None, fl.value() if fl else None)
    G.check_segment_gather(c, *got)
    return got


@pytest.mark.parametrize("F", G.SEG_F)
def test_segment_gather(hb, F):
    for c in [c for c in G.segment_gather_cases() if c["F"] == F]:
        for outs in (("btf",), ("tbf",), ("btf", "tbf")):
            btf, tbf, fl = run_seg(hb, c, outs)
            assert fl == int(c["name"].endswith("all"))  # 1 with a frame outside the pool, still 0 without
        run_seg(hb, c, flag=False)  # a NULL flag word is accepted


def test_segment_gather_misaligned_pointers_take_the_scalar_kernel(hb):
    """F = 8 with one of pool / out_btf / out_tbf 4 bytes past a 16-byte boundary, then all three: V = 1 runs and gives the
    aligned (V = 4) run's values bit for bit."""
    for c in [c for c in G.segment_gather_cases() if c["F"] == 8 and c["name"].endswith("all")]:
        base = run_seg(hb, c)
        for mis in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
            got = run_seg(hb, c, mis=mis)
            G.same_bits(got[0], base[0], "%s mis=%r batch-major" % (c["name"], mis))
            G.same_bits(got[1], base[1], "%s mis=%r time-major" % (c["name"], mis))
            assert got[2] == base[2] == 1
        for outs, mis in ((("btf",), (0, 1, 0)), (("tbf",), (0, 0, 1)), (("tbf",), (1, 0, 0))):  # ... with the other output NULL
            run_seg(hb, c, outs, mis=mis)


# ---------------------------------------------------------------------------------------------
# mu2_accumulate / mu2_finalize
# ---------------------------------------------------------------------------------------------
def run_accumulate(hb, c, split=None):
    N, S, D = c["N"], c["S"], c["D"]
    zsum, cnt = Out(S * D, start=0.0), Out(S, start=0.0)  # accumulators: zeroed by the caller
    for a, b in ((0, N),) if split is None else ((0, split), (split, N)):
        z, idx = In(c["z"][a:b]), In(c["idx"][a:b])
        hb._call("fhvae_mu2_accumulate", z.ptr, idx.ptr, zsum.ptr, cnt.ptr, b - a, S, D)
    return G.check_accumulate(c, zsum.get(S, D), cnt.get())


@pytest.mark.parametrize("N,S,D", G.ACC_SHAPES)
def test_mu2_accumulate(hb, N, S, D):
    c = [c for c in G.accumulate_cases() if (c["N"], c["S"], c["D"]) == (N, S, D)][0]
    shares = [run_accumulate(hb, c)]
    if N > 1:
        shares += [run_accumulate(hb, c, split=N // 3), run_accumulate(hb, c, split=N - 1)]
    print("measured mu2_accumulate %s: worst share of the bound %.3f" % (c["name"], max(shares)))


@pytest.mark.parametrize("N,S,D", G.ACC_SHAPES)
def test_mu2_finalize(hb, N, S, D):
    for c in [c for c in G.finalize_cases() if (c["S"], c["D"]) == (S, D)]:
        zsum, cnt, mu2 = In(c["zsum"]), In(c["cnt"]), Out(S * D)
        hb._call("fhvae_mu2_finalize", zsum.ptr, cnt.ptr, mu2.ptr, S, D, float(c["ratio"]))
        got = mu2.get(S, D)
        G.check_finalize(c, got)
        assert (G.bits(got[c["cnt"] == 0]) == 0).all()  # rows without segments: +0, whatever their zsum holds


# ---------------------------------------------------------------------------------------------
# to_time_major / cast_bf16
# ---------------------------------------------------------------------------------------------
def run_ttm(hb, c, dtype, copy, mis=(0, 0, 0)):
    B, T, F = c["x"].shape
    n = B * T * F
    x = In(c["x"], mis[0])
    o = Out(n, torch.float32 if dtype == "f32" else torch.int16, mis[1])
    of = Out(n, mis=mis[2]) if copy else None
    hb._call("fhvae_to_time_major", x.ptr, o.ptr, ptr(of), B, T, F, hb.F32 if dtype == "f32" else hb.BF16)
    got = (o.get(T, B, F) if dtype == "f32" else None, u16(o.get(T, B, F)) if dtype == "bf16" else None, of.get(T, B, F) if of else None)
    G.check_to_time_major(c, *got)
    return got


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B,T,F", G.TTM_SHAPES)
def test_to_time_major(hb, B, T, F, dtype):
    c = [c for c in G.to_time_major_cases() if c["x"].shape == (B, T, F)][0]
    for copy in (False, True):
        run_ttm(hb, c, dtype, copy)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_to_time_major_misaligned_pointers_take_the_scalar_kernel(hb, dtype):
    """F = 12 with x_btf, x_tbf or x_tbf_f32 one element past a 16-byte boundary (4 bytes of f32, 2 bytes of bf16)."""
    c = [c for c in G.to_time_major_cases() if c["x"].shape[2] == 12][0]
    base = run_ttm(hb, c, dtype, True)
    for mis in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        got = run_ttm(hb, c, dtype, True, mis)
        for a, b in zip(got, base):
            assert (a is None) == (b is None) and (a is None or np.array_equal(a.view(np.uint8), b.view(np.uint8))), mis
    for mis in ((1, 0, 0), (0, 1, 0)):
        run_ttm(hb, c, dtype, False, mis)


def run_cast(hb, c):
    R_, C_ = c["x"].shape
    for want_d, want_t in ((True, False), (False, True), (True, True)):
        x = In(c["x"])
        d = Out(R_ * C_, torch.int16) if want_d else None
        dt = Out(R_ * C_, torch.int16) if want_t else None
        hb._call("fhvae_cast_bf16", x.ptr, ptr(d), ptr(dt), R_, C_)
        G.check_cast(c, u16(d.get(R_, C_)) if d else None, u16(dt.get(C_, R_)) if dt else None)


@pytest.mark.parametrize("R_,C_", G.CAST_SHAPES)
def test_cast_bf16(hb, R_, C_):
    run_cast(hb, [c for c in G.cast_cases() if c["x"].shape == (R_, C_)][0])


def test_cast_bf16_denormals(hb):
    """f32 denormals are rounded to nearest even like every other value (0x00008000 -> 0, 0x00018000 -> 0x0002), not flushed:
    what torch's conversion, and with it rb() of oracle/lstm_lp_ref.py, does.  The kernels run with f32 denormals enabled
    (float_denorm_mode_32 = 3 in the code object) and convert with v_cvt_pk_bf16_f32."""
    run_cast(hb, G.cast_denormal_case())


# ---------------------------------------------------------------------------------------------
# mu2_gather_fwd
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,D", G.GATHER_SHAPES)
def test_mu2_gather_fwd(hb, B, S, D):
    for c in [c for c in G.gather_cases() if c["idx"].shape[0] == B and c["table"].shape == (S, D)]:
        for with_flag in (True, False):
            table, idx, out, fl = In(c["table"]), In(c["idx"]), Out(B * D), Flag() if with_flag else None
            hb._call("fhvae_mu2_gather_fwd", table.ptr, idx.ptr, c["off"], out.ptr, B, S, D, ptr(fl))
            got = out.get(B, D)
            G.check_gather(c, got, fl.value() if fl else None)
            if fl:
                assert fl.value() == int(c["name"].endswith("outside"))
            s = c["idx"] - c["off"]
            assert (G.bits(got[(s < 0) | (s >= S)]) == 0).all()  # rows outside the shard: +0


# ---------------------------------------------------------------------------------------------
# loss_fwd / loss_bwd
# ---------------------------------------------------------------------------------------------
def run_loss(hb, c, fl):
    lb, qy, out = In(c["lb"]), In(np.asarray([c["log_qy"]], np.float32)), Out(1)
    hb._call("fhvae_loss_fwd", lb.ptr, qy.ptr, float(c["alpha"]), out.ptr, c["B"], ptr(fl))
    return out.get()[0]


@pytest.mark.parametrize("B", G.LOSS_B)
def test_loss_fwd(hb, B):
    shares = []
    for c in [c for c in G.loss_cases() if c["B"] == B]:
        fl = Flag()
        loss = run_loss(hb, c, fl)
        shares.append(G.check_loss_fwd(c, loss, fl.value()))
        assert fl.value() == int(c["poison"] is not None)
        G.check_loss_fwd(c, run_loss(hb, c, None), None)  # a NULL word is accepted
    print("measured loss_fwd B=%d: worst share of the bound %.3f" % (B, max(shares)))


def test_loss_fwd_nan_word_is_sticky(hb):
    cases = {c["name"]: c for c in G.loss_cases()}
    fl = Flag()
    for name, want in (("B257-a10-clean", 0), ("B257-a10-nan256", 1), ("B257-a10-clean", 1), ("B4099-a10-clean", 1)):
        loss = run_loss(hb, cases[name], fl)
        assert fl.value() == want and np.isnan(loss) == ("nan" in name), name


@pytest.mark.parametrize("B", G.LOSS_B)
def test_loss_bwd(hb, B):
    for c in [c for c in G.loss_bwd_cases() if c["B"] == B]:
        for with_qy in (True, False):
            g = In(np.asarray([c["g"]], np.float32)) if c["g"] is not None else None
            d_lb, d_qy = Out(B), Out(1) if with_qy else None
            hb._call("fhvae_loss_bwd", ptr(g), float(c["alpha"]), d_lb.ptr, ptr(d_qy), B)
            G.check_loss_bwd(c, d_lb.get(), d_qy.get() if d_qy else None)  # (get: nothing written past d_lower_bound[B - 1])


# ---------------------------------------------------------------------------------------------
# the row shard's exchange helpers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D", G.PACK_SHAPES)
def test_shard_pack_and_unpack(hb, B, D):
    c = [c for c in G.pack_cases() if c["q"].shape == (B, D)][0]
    q, idx, out = In(c["q"]), In(c["idx"]), Out(B * (D + 1))
    hb._call("fhvae_shard_pack", q.ptr, idx.ptr, out.ptr, B, D)
    G.check_pack(c, out.get(B, D + 1).view(np.uint32))
    # unpack reads a buffer the ORACLE packed: a pack and an unpack that agree with each other and are both wrong do not pass
    pk = In(R.shard_pack_ref(c["q"], c["idx"]).view(np.float32))
    uq, ui = Out(B * D), Out(B, torch.int64)
    hb._call("fhvae_shard_unpack", pk.ptr, uq.ptr, ui.ptr, B, D)
    G.check_unpack(c, uq.get(B, D), ui.get())


@pytest.mark.parametrize("N,D", G.BWD_SHAPES)
def test_shard_bwd_pack(hb, N, D):
    for c in [c for c in G.bwd_pack_cases() if (c["N"], c["D"]) == (N, D)]:
        dq = In(c["dq_all"]) if c["dq_all"] is not None else None
        dmu2 = In(c["dmu2_local"]) if c["dmu2_local"] is not None else None  # (n_own = 0: an empty range of a real allocation)
        out = Out(N * 2 * D)
        hb._call("fhvae_shard_bwd_pack", ptr(dq), float(c["dq_scale"]), ptr(dmu2), c["own0"], c["n_own"], out.ptr, N, D)
        G.check_bwd_pack(c, out.get(N, 2 * D))  # every element written: none is still NaN


@pytest.mark.parametrize("N,D", G.BWD_SHAPES)
def test_shard_bwd_unpack(hb, N, D):
    for c in [c for c in G.bwd_unpack_cases() if (c["N"], c["D"]) == (N, D)]:
        buf = In(c["buf"])
        dq = Out(c["n_own"] * D) if c["want_dq"] else None  # the rows of dq_local outside the own range do not exist
        dm = Out(N * D) if c["want_dmu2"] else None
        hb._call("fhvae_shard_bwd_unpack", buf.ptr, c["own0"], c["n_own"], ptr(dq), ptr(dm), N, D)
        G.check_bwd_unpack(c, dq.get(c["n_own"], D) if dq else None, dm.get(N, D) if dm else None)
