"""The three matrix-product kernels -- csrc/proj.hip (fhvae_proj_bf16), csrc/wgrad.hip (fhvae_wgrad_bf16 / fhvae_wgrad_f32 and the
grouped launch behind fhvae_lstm_param_grads_multi) and the generic engine of csrc/gemm.hip / csrc/gemm_core.h behind
hip_binding.raw_linear_fwd / raw_linear_bwd -- against the float64 oracle of the same operands (oracle/gemm_ref.py), at every
launch branch.  The comparator and its constants are the heads' (tests/head_elbo_compare.py: check_contraction, check_bias,
HEAD["bf16"] / HEAD["f32"]): per element |err| <= c U sqrt(K) (|A| |B| + |c0| + |bias|), 64 x 64 tile bins.

The case tables below are chosen with the library's launch plans (tests/matmul_plan_sweep.py); tests/test_gemm_oracle_cpu.py
proves on the CPU that they reach every compiled branch, and every GPU case asserts the branch it was chosen for.

Every case: the operands are the leading rows and columns of wider and taller allocations whose every other element is NaN
(leading-dimension padding, k-rows past K of KM operands, k-columns [K, ld) of KC operands: what the kernel may address but
must not use), and the outputs are a row (and column) range of a buffer filled with a sentinel that must come back untouched.
Operand views start at column 0 of their allocation: the stand-alone entries have no a_col0, so the buffer range of an offset
view would run past the allocation.

Measured on an MI355X (this file, every case; max / mean of the ratio to U sqrt(K) absprod):
  proj                      max 0.28 (32775 x 160 x 64, BM 160 BN 256) / mean 0.013; worst bin 1.41 x its median
  wgrad bf16, one call      max 1.00 (K = 1) / mean 0.14;  after the second call max 1.99 (K = 1) / mean 0.19
  wgrad f32, one call       max 1.72 (K = 1) / mean 0.34;  after the second call max 2.25 (K = 1) / mean 0.46
  wgrad grouped (bf16)      max 0.19 (K = 64, 1024 x 132, one slice) / mean 0.013
  linear y / dx / dw        max 0.79 (4100 x 68 x 2052) / 0.61 / 0.44, means <= 0.042; worst bin 1.55 x its median
  linear db (check_bias)    max 1.18 / mean 0.18
  |signed mean| <= 0.009 on every contraction, 0.056 on db; no sentinel touched, every output finite.
The maxima sit at K = 1, where the summation model's worst case is (K + 1) / sqrt(K) = 2 roundings' worth per call (the product,
for f32 operands, and the addition into c0; a second call adds as much again): the kernels meet the CPU emulation's floor
(1.00 / 1.76, tests/test_gemm_oracle_cpu.py) and fall with K from there.
"""
import ctypes as C

import pytest
import torch

import matmul_plan_sweep as GP
import head_elbo_compare as HC
from oracle import gemm_ref as GR

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
NAN = float("nan")


@pytest.fixture(scope="module")
def hb():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding

    hip_binding.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return hip_binding


# ---------------------------------------------------------------------------------------------
# buffers (device-agnostic: the CPU file runs its emulated kernel through the same ones)
# ---------------------------------------------------------------------------------------------
def rup(n, m):
    return -(-n // m) * m


def padded(rows, cols, ld, pad_rows, dtype, gen, dev, scale=1.0):
    """randn * scale [rows, cols] as the leading rows and columns of a [rows + pad_rows, ld] allocation that is NaN everywhere
    else.  Returns the view (it starts at the allocation's first element)."""
    assert ld >= cols and pad_rows >= 1
    full = torch.full((rows + pad_rows, ld), NAN, dtype=dtype, device=dev)
    full[:rows, :cols] = (torch.randn(rows, cols, generator=gen) * scale).to(dtype).to(dev)
    return full[:rows, :cols]


def canary(rows, cols, r0, c0, extra_cols, dev, gen=None):
    """A [rows, cols] output at (r0, c0) of a [rows + 2 r0, c0 + cols + extra_cols] buffer of SENTINEL.  gen: the output starts as
    randn (an accumulator's c0), else NaN (every element must be written).  Returns (view, whole buffer, start value copy)."""
    full = torch.full((rows + 2 * r0, c0 + cols + extra_cols), SENTINEL, dtype=torch.float32, device=dev)
    view = full[r0:r0 + rows, c0:c0 + cols]
    start = torch.randn(rows, cols, generator=gen).to(dev) if gen is not None else torch.full((rows, cols), NAN, device=dev)
    view.copy_(start)
    return view, full, start


def canary_bad(view, full, label):
    """Nothing outside `view` was written."""
    t = full.clone()
    r0, c0 = (view.data_ptr() - full.data_ptr()) // 4 // full.stride(0), (view.data_ptr() - full.data_ptr()) // 4 % full.stride(0)
    t[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = SENTINEL
    n = int((t != SENTINEL).sum().item())
    return ["%s: %d elements outside the output were written" % (label, n)] if n else []


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(hash(tuple(int(k) for k in key)) & 0x7FFFFFFF)
    return g


# ---------------------------------------------------------------------------------------------
# proj.hip: (M, N, K, BM, BN) -- every instantiated (BM, BN), more than one round, two column tiles, the BM = 64 edges
# ---------------------------------------------------------------------------------------------
PROJ_CASES = [
    (16392, 4, 64, 96, 128), (24585, 100, 192, 128, 128), (32769, 64, 64, 160, 128), (40993, 128, 128, 192, 128),
    (49157, 36, 64, 224, 128), (57347, 124, 64, 256, 128),
    (16391, 132, 64, 96, 256), (24583, 256, 128, 128, 256), (32775, 160, 64, 160, 256), (40999, 252, 192, 192, 256),
    (49155, 136, 64, 224, 256), (57351, 200, 64, 256, 256),
    (65525, 136, 64, 256, 256),   # 256 tiles: the last single round
    (8205, 512, 64, 96, 256),     # two column tiles
    (12289, 516, 128, 160, 256),  # a ragged second column tile (4 columns)
    (70000, 64, 64, 96, 128),     # 730 tiles: three rounds
    (63, 4, 64, 64, 128), (65, 128, 64, 64, 128), (33, 260, 320, 64, 256),  # BM = 64: M % BM = BM - 1, 1; two column tiles, odd K / 64
]


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("M,N,K,bm,bn", PROJ_CASES)
def test_proj_against_the_oracle(hb, M, N, K, bm, bn, bias):
    assert GP.proj_plan(M, N)[:2] == (bm, bn)
    g = _gen(1, M, N, K)
    a = padded(M, K, K + 8, 3, torch.bfloat16, g, "cuda")
    b = padded(N, K, K + 16, 2, torch.bfloat16, g, "cuda")
    bv = torch.randn(N, generator=g).cuda() if bias else None
    out, full, _ = canary(M, N, 1, 4, 4, "cuda")
    hb.proj_bf16(a, b, bv, out=out)
    want, ab = GR.contraction(a, b, True, True, bias=bv)
    label = "proj %dx%dx%d BM %d BN %d%s" % (M, N, K, bm, bn, " +bias" if bias else "")
    bad = HC.check_contraction(out, want, ab, K, HC.HEAD["bf16"], label) + canary_bad(out, full, label)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# wgrad.hip, stand-alone: (K, M, N, output column offset, extra output columns); both element types
# ---------------------------------------------------------------------------------------------
WGRAD_CASES = [
    (1, 256, 256, 0, 0), (7, 40, 24, 0, 0), (100, 300, 130, 0, 0), (70, 300, 260, 0, 0), (129, 520, 129, 0, 0),
    (197, 256, 128, 0, 0), (576, 264, 72, 0, 0),
    (100, 300, 130, 3, 5), (197, 256, 128, 3, 5),  # ldc > N, one per tile class: nothing outside C[:M, :N] is written
    # what the coverage test asks for beyond those (tests/test_gemm_oracle_cpu.py lists the properties per element type and tile class):
    # K % BK in {0, 1, BK - 1} for BK = 64 and 32, a short last slice, a grid of 16 or more that is no multiple of 8
    (1537, 264, 24, 0, 0), (63, 40, 24, 0, 0), (2047, 40, 520, 0, 0), (64, 40, 130, 0, 0), (383, 40, 520, 0, 0),
]
WG_DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}


def wgrad_lds(M, N):
    """Padded leading dimensions (multiples of 16 bytes for either element): M = 300 sits under lda = 312."""
    return rup(M, 8) + 8, rup(N, 8) + 16


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("K,M,N,col0,extra", WGRAD_CASES)
def test_wgrad_against_the_oracle(hb, K, M, N, col0, extra, dt):
    g = _gen(2, K, M, N)
    lda, ldb = wgrad_lds(M, N)
    a = padded(K, M, lda, 3, WG_DTYPES[dt], g, "cuda")
    b = padded(K, N, ldb, 3, WG_DTYPES[dt], g, "cuda")
    c, full, c0 = canary(M, N, 1, col0, extra, "cuda", gen=g)
    fn = hb.wgrad_bf16_ if dt == "bf16" else hb.wgrad_f32_
    fn(c, a, b)
    first = c.clone()
    fn(c, a, b)  # accumulates: a second call adds the product again
    want, ab = GR.contraction(a, b, False, False, c0=c0)
    (BN, sk, grid, per, _), = GP.wgrad_plan([(K, M, N)], dt == "bf16")
    label = "wgrad %s K %d %dx%d BN %d split %d grid %d ldc+%d" % (dt, K, M, N, BN, per[0]["splitk"], grid, col0 + extra)
    bad = HC.check_contraction(first, want, ab, K, HC.HEAD[dt], label)
    bad += HC.check_contraction(c, 2 * want - c0.double(), 2 * ab - c0.double().abs(), K, HC.HEAD[dt], label + " twice")
    bad += canary_bad(c, full, label)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# wgrad.hip, the grouped launch (bf16): problems (K, M, N, name of C); an equal name is the same C with the same operands
# ---------------------------------------------------------------------------------------------
WIDE = [(2048, 512, 256, "w0"), (200, 512, 256, "w1"), (64, 1024, 132, "w2"), (1000, 256, 520, "w3"), (2048, 512, 256, "w0")]
NARROW = [(2048, 512, 80, "n0"), (130, 64, 8, "n1"), (777, 320, 128, "n2"), (2048, 512, 80, "n0")]
GROUPS = {
    "wide": WIDE,                # sk 4; (200, ..) clipped to 2 slices, (64, ..) one slice beside split ones; 36 workgroups; shared_c
    "narrow": NARROW,
    "both": WIDE + NARROW,       # the two tile classes of one call
    "seventeen": [(300 + 10 * i, 64, 32, "s%d" % i) for i in range(17)],  # chunks of kMaxWgProblems = 16 + 1
}
PAIR = {"K": 600, "D": 40, "N": 72}  # a_col0 = 0 and D into one [K, 2D (+ pad)] operand, as the heads build it


def _grouped_run(hb, descs, keep, through_queue):
    if through_queue:
        hb.flush_param_grads()  # (whatever an earlier test left queued)
        hb._DEFER["extra"].extend((x, keep) for x in descs)
        hb.flush_param_grads()
    else:
        xs = (hb.WgradDesc * len(descs))(*descs)
        hb._call("fhvae_lstm_param_grads_multi", None, 0, xs, len(descs))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_wgrad_grouped_launch_against_the_oracle(hb, name):
    probs = GROUPS[name]
    lib = hb.load_library()
    bufs, descs, keep = {}, [], []
    for i, (K, M, N, cn) in enumerate(probs):
        if cn not in bufs:
            g = _gen(3, K, M, N, i)
            lda, ldb = wgrad_lds(M, N)
            a = padded(K, M, lda, 2, torch.bfloat16, g, "cuda")
            b = padded(K, N, ldb, 2, torch.bfloat16, g, "cuda")
            bufs[cn] = (a, b) + canary(M, N, 1, 3, 4, "cuda", gen=g) + (K, [])
        a, b, c = bufs[cn][:3]
        bufs[cn][6].append(i)
        d = hb.WgradDesc(a.data_ptr(), a.stride(0), 0, b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0), M, N, K)
        assert lib.fhvae_wgrad_desc_ok(C.byref(d)) == 1
        descs.append(d)
        keep.append((a, b, c))
    _grouped_run(hb, descs, keep, through_queue=name != "both")
    plan = {i: (l[0], l[3][j]) for l in GP.wgrad_plan(probs, True) for j, i in enumerate(l[4])}
    bad = []
    for cn, (a, b, c, full, c0, K, idx) in bufs.items():
        n = len(idx)  # a duplicated C goes against n times the product
        want, ab = GR.contraction(a, b, False, False)
        BN, d = plan[idx[0]]
        label = "grouped %s %s K %d %dx%d BN %d split %d x%d" % (name, cn, K, c.shape[0], c.shape[1], BN, d["splitk"], n)
        bad += HC.check_contraction(c, n * want + c0.double(), n * ab + c0.double().abs(), K, HC.HEAD["bf16"], label)
        bad += canary_bad(c, full, label)
    assert not bad, bad


def test_wgrad_grouped_pair_with_a_col0(hb):
    K, D, N = PAIR["K"], PAIR["D"], PAIR["N"]
    lib = hb.load_library()
    g = _gen(4, K, D, N)
    gp = padded(K, 2 * D, 2 * D + 8, 2, torch.bfloat16, g, "cuda")  # [g_mu | g_lv | pad]
    h = padded(K, N, N + 8, 2, torch.bfloat16, g, "cuda")
    outs = [canary(D, N, 1, 3, 4, "cuda", gen=g) for _ in range(2)]
    descs = [hb.WgradDesc(gp.data_ptr() + 2 * i * D, gp.stride(0), i * D, h.data_ptr(), h.stride(0), outs[i][0].data_ptr(),
                          outs[i][0].stride(0), D, N, K) for i in range(2)]
    assert all(lib.fhvae_wgrad_desc_ok(C.byref(d)) == 1 for d in descs)
    _grouped_run(hb, descs, (gp, h, outs), through_queue=True)
    bad = []
    for i, (c, full, c0) in enumerate(outs):
        want, ab = GR.contraction(gp[:, i * D:(i + 1) * D], h, False, False, c0=c0)
        label = "grouped pair a_col0 %d K %d %dx%d" % (i * D, K, D, N)
        bad += HC.check_contraction(c, want, ab, K, HC.HEAD["bf16"], label) + canary_bad(c, full, label)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# the generic engine behind hip_binding.linear: (M, K, N, the forward's kernel, its LDS-DMA tiles, dw's K slices)
# ---------------------------------------------------------------------------------------------
LINEAR_CASES = [
    (128, 256, 128, "swap+dma", 4, 1),     # mainloop_glds on every tile
    (200, 384, 136, "swap+dma", 6, 1),     # ... on 6 of 12 tiles, the staged main loop on the ragged ones
    (1088, 132, 1024, "swap", 0, 4),       # 272 tiles: the swapped kernel without the DMA instantiation; dw split 4
    (4100, 68, 2052, "swap", 0, 8),        # 128 x 128 tiles (561, ragged), K tail 4; dw split 8
    (1024, 128, 64, "swap+dma", 16, 4),    # dw split 4 over 2 tiles
    (96, 64, 64, "swap", 0, 1),            # CH = 8 (K <= 64) ...
    (96, 68, 64, "swap+dma", 0, 1),        # ... and CH = 32 one chunk above it
    (100, 64, 70, "swap", 0, 1),           # N % 4 != 0: the swapped epilogue's scalar stores; dx and dw on gemm_slow_kernel
    (640, 1600, 128, "swap+dma", 0, 2),    # the FC model's first layer at B = 640: dw split 2
]
LINEAR_PAD = 4  # ld = columns + 4 for x, w and dy


def linear_plans(M, K, N, relu):
    return GP.linear_plans(M, K, N, relu, K + LINEAR_PAD, K + LINEAR_PAD, N + LINEAR_PAD)


def _linear_inputs(M, K, N):
    g = _gen(5, M, K, N)
    x = padded(M, K, K + LINEAR_PAD, 2, torch.float32, g, "cuda")
    w = padded(N, K, K + LINEAR_PAD, 1, torch.float32, g, "cuda", scale=K ** -0.5)
    dy = padded(M, N, N + LINEAR_PAD, 2, torch.float32, g, "cuda")
    return g, x, w, torch.randn(N, generator=g).cuda(), dy


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,K,N,kernel,dma,dw_split", LINEAR_CASES)
def test_linear_against_the_oracle(hb, M, K, N, kernel, dma, dw_split, relu):
    pl = linear_plans(M, K, N, relu)
    assert (pl["y"][4], pl["y"][5]) == (kernel, dma) and (pl["dw"] == "slow" or pl["dw"][2] == dw_split)
    g, x, w, b, dy = _linear_inputs(M, K, N)
    label = "linear %dx%dx%d %s%s" % (M, K, N, kernel, " relu" if relu else "")
    y = hb.raw_linear_fwd(x, w, b, relu)
    want, ab = GR.linear_fwd(x, w, b, relu)
    bad = HC.check_contraction(y, want, ab, K, HC.HEAD["f32"], label + " y")
    # the same launch into a column range of a wider buffer (ld % 4 and N % 4 as before: the same epilogue)
    y2, full, _ = canary(M, N, 1, 4, 4, "cuda")
    hb._call("fhvae_linear_fwd", x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), b.data_ptr(), y2.data_ptr(), y2.stride(0),
             None, M, K, N, int(relu), hb.F32)
    bad += canary_bad(y2, full, label + " y (ldy > N)")
    if not torch.equal(y2, y):
        bad.append(label + ": y differs between ldy = N and ldy > N")
    # backward from the kernel's own y (chained); dw and db accumulate into nonzero sinks
    dw, dw_full, dw0 = canary(N, K, 1, 0, 0, "cuda", gen=g)
    db = torch.randn(N, generator=g).cuda()
    db0 = db.clone()
    dx, _, _ = hb.raw_linear_bwd(x, w, y if relu else None, dy, relu, dw_sink=dw, db_sink=db)
    o = GR.linear_bwd(x, w, y, dy, relu, dw0=dw0, db0=db0)
    bad += HC.check_contraction(dx, o["dx"], o["a_dx"], N, HC.HEAD["f32"], label + " dx")
    bad += HC.check_contraction(dw, o["dw"], o["a_dw"], M, HC.HEAD["f32"], label + " dw split %s" % (pl["dw"] if pl["dw"] == "slow" else pl["dw"][2]))
    bad += HC.check_bias(db, o["db"], o["a_db"], HC.HEAD["f32"], label + " db")
    bad += canary_bad(dw, dw_full, label + " dw")
    assert not bad, bad


@pytest.mark.parametrize("M,K,N,relu", [(200, 384, 136, True), (100, 64, 70, False)])
def test_linear_dx_accumulates_into_dx_out(hb, M, K, N, relu):
    """dx_out= : dx_accumulate (mode 1) on the staged kernel and on gemm_slow_kernel."""
    g, x, w, b, dy = _linear_inputs(M, K, N)
    y = hb.raw_linear_fwd(x, w, b, relu)
    dx, full, dx0 = canary(M, K, 1, 0, 0, "cuda", gen=g)
    hb.raw_linear_bwd(x, w, y if relu else None, dy, relu, need_dw=False, need_db=False, dx_out=dx)
    o = GR.linear_bwd(x, w, y, dy, relu, dx0=dx0)
    label = "linear %dx%dx%d dx_out%s" % (M, K, N, " relu" if relu else "")
    bad = HC.check_contraction(dx, o["dx"], o["a_dx"], N, HC.HEAD["f32"], label) + canary_bad(dx, full, label)
    assert not bad, bad
