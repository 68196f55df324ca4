"""The Gaussian heads (K2: gemm.hip, proj.hip, wgrad.hip) and the fused lower bound (K3: loss.hip) against the float64 oracle of
their own arithmetic (oracle/head_elbo_ref.py), with one comparator and one set of constants per mode (tests/head_elbo_compare.py).
Most cases call the C ABI directly (hip_binding.load_library()), which reaches branches the autograd binding does not choose;
each says which branch it reaches and the condition that selects it.  The config-shape cases run end to end through
hip_binding.gauss_head + hip_binding.elbo.  The oracle runs in float64 on the GPU; every case prints its measurements."""
import ctypes as C

import pytest
import torch

import head_elbo_compare as HC
from oracle import head_elbo_ref as HR

pytestmark = pytest.mark.gpu

NAMES = HR.UPSTREAMS
GRADS = ("d_z1_mu", "d_z1_lv", "d_z2_mu", "d_z2_lv", "d_mu2")


@pytest.fixture(scope="module")
def hb():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding

    hip_binding.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return hip_binding


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _offset(t: torch.Tensor, elems: int) -> torch.Tensor:
    """A device copy of t whose base sits `elems` elements past a 256-byte aligned allocation (4 bytes for one f32, 8 for four
    bf16): same values, contiguous, misaligned for the 16-byte vector paths."""
    buf = torch.empty(t.numel() + elems, dtype=t.dtype, device="cuda")
    v = buf[elems:].view(t.shape)
    v.copy_(t)
    return v


# ---------------------------------------------------------------------------------------------
# lower bound (fhvae_elbo_fwd / fhvae_elbo_bwd)
# ---------------------------------------------------------------------------------------------
def _elbo_gpu(hb, inp, tm, misalign, detach, ups, nsegs, pair_ld=None):
    """Run the two kernels on inp (batch-major CPU tensors) laid out time-major (tm) or batch-major on the device; misalign:
    x / x_mu / x_lv 4 bytes off 16-byte alignment.  pair_ld: the pair kernel's ld_pair (time-major only).  Returns (fwd dict,
    bwd dict with batch-major d_x, pair extras)."""
    lib = hb.load_library()
    B, T, F = inp["x"].shape
    lay = (lambda t: t.transpose(0, 1).contiguous()) if tm else (lambda t: t.contiguous())
    dv = (lambda t: _offset(lay(t).cuda(), 1)) if misalign else (lambda t: lay(t).cuda())
    x, xm, xl = dv(inp["x"]), dv(inp["x_mu"]), dv(inp["x_lv"])
    z = [t.cuda().contiguous() for t in inp["z"]]
    strides = (F, B * F) if tm else (T * F, F)
    ns = nsegs.cuda() if isinstance(nsegs, torch.Tensor) else nsegs
    outs = [torch.empty(B, device="cuda") for _ in range(5)]
    d = hb.ElboDesc()
    hb._fill_elbo_desc(d, x, strides, xm, xl, strides, *z, ns, B, T, F)
    d.lower_bound, d.log_px_z, d.neg_kld_z1, d.neg_kld_z2, d.log_pmu2 = (_p(o) for o in outs)
    assert lib.fhvae_elbo_fwd(C.byref(d), _st()) == 0
    bd = hb.ElboBwdDesc()
    hb._fill_elbo_desc(bd.f, x, strides, xm, xl, strides, *z, ns, B, T, F)
    gs = {k: (v.cuda() if v is not None else None) for k, v in ups.items()}
    bd.g_lower_bound, bd.g_log_px_z, bd.g_neg_kld_z1, bd.g_neg_kld_z2, bd.g_log_pmu2 = (_p(gs.get(k)) for k in NAMES)
    bd.reference_detach = int(detach)
    dxm, dxl = (torch.full_like(x, float("nan")) for _ in range(2))
    dz = [torch.empty_like(t) for t in z]
    bd.d_x_mu, bd.d_x_lv = _p(dxm), _p(dxl)
    bd.d_z1_mu, bd.d_z1_lv, bd.d_z2_mu, bd.d_z2_lv, bd.d_mu2 = (_p(t) for t in dz)
    extra = {}
    if pair_ld is not None:
        extra["pair"] = torch.full((T * B, pair_ld), float("nan"), device="cuda", dtype=torch.bfloat16)
        extra["colsum"] = torch.full((int(lib.fhvae_elbo_colsum_rows(B)), 2 * F), float("nan"), device="cuda")
        bd.d_x_pair_lp, bd.ld_pair, bd.d_x_colsum = _p(extra["pair"]), pair_ld, _p(extra["colsum"])
    assert lib.fhvae_elbo_bwd(C.byref(bd), _st()) == 0
    torch.cuda.synchronize()
    un = (lambda t: t.transpose(0, 1)) if tm else (lambda t: t)
    fwd = dict(zip(NAMES, outs))
    bwd = dict(zip(GRADS, dz))
    bwd["d_x_mu"], bwd["d_x_lv"] = (None, None) if detach else (un(dxm), un(dxl))
    return fwd, bwd, extra


def _elbo_compare(got_f, got_b, want_f, want_b, B, T, F, label):
    bad = []
    for n in NAMES:
        bad += HC.check_elementwise(got_f[n], want_f[n], want_f["a_" + n], HC.ELBO, label + " " + n, bins=(("row", torch.arange(B)),))
    for n in GRADS:
        bad += HC.check_elementwise(got_b[n], want_b[n], want_b["a_" + n], HC.ELBO, label + " " + n)
    if want_b["d_x_mu"] is not None:
        for n in ("d_x_mu", "d_x_lv"):
            bad += HC.check_elementwise(got_b[n], want_b[n], want_b["a_" + n], HC.ELBO, label + " " + n, bins=HC.row_time_bins(B, T, F))
    return bad


def _dev(inp):
    return {k: ([t.cuda() for t in v] if isinstance(v, list) else {a: b.cuda() for a, b in v.items()} if isinstance(v, dict)
                else v.cuda()) for k, v in inp.items()}


# (B, T, F, D1, D2, time-major, misaligned, regime).  Vector path: F % 4 == 0, every stride % 4 == 0 and 16-byte aligned bases
# (elbo_fwd_kernel `vec`, loss.hip:102-103; elbo_bwd_kernel loss.hip:210-211); scalar path otherwise: F % 4 != 0 or a base 4 bytes
# off.  D1 / D2 = 65 and 128 run the 64-lane loops (loss.hip:126, 131, 181, 187) twice.
ELBO_CASES = [
    (7, 3, 12, 8, 32, False, False, "typical"),     # vector, batch-major
    (33, 20, 80, 32, 8, True, False, "lv_neg"),     # vector, time-major
    (5, 4, 7, 65, 128, False, False, "typical"),    # scalar: F % 4 != 0
    (6, 5, 9, 128, 65, True, False, "lv_pos"),      # scalar: F % 4 != 0, time-major
    (260, 20, 80, 65, 32, False, True, "prior"),    # scalar: bases 4 bytes off 16-byte alignment
    (131, 20, 80, 32, 128, True, True, "typical"),  # scalar, time-major, misaligned
]


@pytest.mark.parametrize("B,T,F,D1,D2,tm,mis,regime", ELBO_CASES)
def test_elbo_kernels(hb, B, T, F, D1, D2, tm, mis, regime):
    """elbo_fwd_kernel and elbo_bwd_kernel (no pair copy): per-row and scalar num_segs, detach on and off, every upstream
    gradient alone and all five together."""
    inp = HC.elbo_inputs(B, T, F, D1, D2, regime, B * 7 + F)
    di = _dev(inp)
    args = (di["x"], di["x_mu"], di["x_lv"], *di["z"])
    bad = []
    for nsegs in (inp["num_segs"], 37):
        want_f = HR.elbo_ref_fwd(*args, di["num_segs"] if nsegs is inp["num_segs"] else nsegs)
        for detach in (False, True):
            for which in (NAMES,) + tuple((n,) for n in NAMES):
                ups = {k: (inp["ups"][k] if k in which else None) for k in NAMES}
                label = "elbo %s %s ns=%s det=%d up=%s" % ((B, T, F, D1, D2), "tm" if tm else "bm",
                                                           "row" if nsegs is inp["num_segs"] else nsegs, detach, "all" if len(which) > 1 else which[0])
                gf, gb, _ = _elbo_gpu(hb, inp, tm, mis, detach, ups, nsegs)
                want_b = HR.elbo_ref_bwd(*args, di["num_segs"] if nsegs is inp["num_segs"] else nsegs,
                                         {k: (v.cuda() if v is not None else None) for k, v in ups.items()}, detach)
                bad += _elbo_compare(gf, gb, want_f, want_b, B, T, F, label)
    assert not bad, bad[:20]


def _pair_ref(gb, ld):
    """The pair rows' reference: the kernel's own f32 d_x (batch-major) in time-major rows, zero padded (chained)."""
    B, T, F = gb["d_x_mu"].shape
    w = torch.zeros(T * B, ld, dtype=torch.float64, device="cuda")
    w[:, :2 * F] = torch.cat([gb["d_x_mu"], gb["d_x_lv"]], 2).transpose(0, 1).reshape(T * B, 2 * F).double()
    return w


# elbo_bwd_pair_kernel (loss.hip:241-307; fhvae_elbo_bwd takes it when d_x_pair_lp is given, loss.hip:587-597): F4 = F / 4 lanes per
# row, RP = 64 / F4 rows per pass (F = 4: 64; 8: 32; 80: 3; 128: 2; 132 and 256: 1), 2F = 512 fills the LDS row cs[.][512];
# a wave takes passes p0, p0 + 2, ... four at a time (T = 50 at F = 80: 17 passes, each wave loops); odd B leaves the second
# segment slot of the last workgroup empty; ld_pair > 2F writes the zero padding (loss.hip:290-294).
PAIR_CASES = [(3, 1, 4, 72), (33, 20, 8, 16), (257, 50, 80, 192), (65, 40, 128, 256), (31, 20, 132, 320), (17, 50, 256, 512),
              (2047, 20, 80, 160), (1, 1, 256, 520)]


@pytest.mark.parametrize("B,T,F,ld", PAIR_CASES)
def test_elbo_pair_kernel(hb, B, T, F, ld):
    """d_x_mu / d_x_lv, the bf16 pair rows and their padding, the column sums, the latent gradients; then the column sums
    through fhvae_gauss_head_bwd_pair's col_sum path (add_split_kernel, gemm.hip:897-904): bias_from = "f32"."""
    lib = hb.load_library()
    inp = HC.elbo_inputs(B, T, F, 32, 32, "typical", B + T + F)
    di = _dev(inp)
    args = (di["x"], di["x_mu"], di["x_lv"], *di["z"], di["num_segs"])
    gf, gb, ex = _elbo_gpu(hb, inp, True, False, False, inp["ups"], inp["num_segs"], pair_ld=ld)
    want_f = HR.elbo_ref_fwd(*args)
    want_b = HR.elbo_ref_bwd(*args, di["ups"], False)
    label = "pair %s ld=%d" % ((B, T, F), ld)
    bad = _elbo_compare(gf, gb, want_f, want_b, B, T, F, label)
    bad += HC.check_bf16(ex["pair"], _pair_ref(gb, ld), 2 * F, label + " d_x_pair_lp")
    s, a = HR.pair_colsum(want_b["d_x_mu"], want_b["d_x_lv"], want_b["a_d_x_mu"], want_b["a_d_x_lv"])
    bad += HC.check_bias(ex["colsum"].double().sum(0), s, a, HC.HEAD["bf16"], label + " colsum rows")
    D = F
    db_mu, db_lv = torch.full((D,), 0.25, device="cuda"), torch.full((D,), -0.5, device="cuda")
    assert lib.fhvae_gauss_head_bwd_pair(None, 0, None, ld, _p(ex["pair"]), ld, _p(ex["colsum"]), ex["colsum"].shape[0], None, 0, None,
                                         None, _p(db_mu), _p(db_lv), T * B, 64, D, _st()) == 0
    bad += HC.check_bias(torch.cat([db_mu - 0.25, db_lv + 0.5]), s, a, HC.HEAD["bf16"], label + " db via add_split")
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# bf16 head through the ABI
# ---------------------------------------------------------------------------------------------
def _pair_ld(D):
    return (2 * D + 63) // 64 * 64


def _head_lp_gpu(hb, i, ldt_extra=0, h_off=False, want_db=True):
    """The bf16 head's launches one by one, as _GaussHeadLp makes them.  Returns the kernel's tensors."""
    lib = hb.load_library()
    M, K = i["h"].shape
    D = i["w_mu"].shape[0]
    ldg = _pair_ld(D)
    ldt = ldg + ldt_extra
    c = {k: (v.cuda() if v is not None else None) for k, v in i.items()}
    h_lp = c["h"].bfloat16()
    if h_off:
        h_lp = _offset(h_lp, 4)  # 8 bytes off 16-byte alignment
    wl = torch.empty(2 * D, K, device="cuda", dtype=torch.bfloat16)
    wt = torch.full((K, ldt), float("nan"), device="cuda", dtype=torch.bfloat16)
    assert lib.fhvae_head_pair_weights(_p(c["w_mu"]), _p(c["w_lv"]), _p(wl), _p(wt), ldt, D, K, _st()) == 0
    out = torch.empty(M, 2 * D, device="cuda")
    assert lib.fhvae_gauss_head_pair_fwd(_p(h_lp), K, _p(wl), _p(c["b_mu"]), _p(c["b_lv"]), _p(out), 2 * D, M, K, D, _st()) == 0
    r = {"out": out, "h_lp": h_lp}
    lv = out[:, D:]
    if c["eps"] is not None:
        smp, mu_c, lv_c = (torch.empty(M, D, device="cuda") for _ in range(3))
        assert lib.fhvae_gauss_reparam_pair_fwd(_p(out), 2 * D, _p(c["eps"]), _p(smp), _p(mu_c), _p(lv_c), M, D, _st()) == 0
        r.update(sample=smp, mu_c=mu_c, lv_c=lv_c)
        lv = lv_c
    # d_s: a column slice of a wider gradient (cat's backward), row stride 2D + 8
    ds = None
    if c["d_s"] is not None:
        wide = torch.randn(M, 2 * D + 8, device="cuda")
        wide[:, D:2 * D] = c["d_s"]
        ds = wide[:, D:2 * D]
    g_lp = torch.full((M, ldg), float("nan"), device="cuda", dtype=torch.bfloat16)
    db = [torch.full((D,), 0.5, device="cuda"), torch.full((D,), -0.25, device="cuda")] if want_db else [None, None]
    assert lib.fhvae_gauss_reparam_bwd_pair(_p(c["d_mu"]), _p(c["d_lv"]), _p(ds), ds.stride(0) if ds is not None else D, _p(c["eps"]),
                                            _p(lv), lv.stride(0), _p(g_lp), ldg, _p(db[0]), _p(db[1]), M, D, _st()) == 0
    dh = torch.full((M, K), float("nan"), device="cuda")
    dw = [torch.full((D, K), 0.125, device="cuda"), torch.full((D, K), -0.125, device="cuda")]
    assert lib.fhvae_gauss_head_bwd_pair(_p(h_lp), K, _p(wt), ldt, _p(g_lp), ldg, None, 0, _p(dh), K, _p(dw[0]), _p(dw[1]), None, None,
                                         M, K, D, _st()) == 0
    torch.cuda.synchronize()
    r.update(g_lp=g_lp, dh=dh, dW=torch.cat([dw[0] - 0.125, dw[1] + 0.125]), ldg=ldg)
    if want_db:
        r["db"] = torch.cat([db[0] - 0.5, db[1] + 0.25])
    return r


def _head_compare(i, r, mode, label, lv_for_g=None):
    """Every output of a head against the oracle, chained on the kernel's own intermediates."""
    lp = mode == "bf16"
    k = HC.HEAD[mode]
    M, K = i["h"].shape
    D = i["w_mu"].shape[0]
    c = {a: (v.cuda() if v is not None else None) for a, v in i.items()}
    f = HR.head_ref_fwd(c["h"], c["w_mu"], c["b_mu"], c["w_lv"], c["b_lv"], None, lp=lp)
    bad = HC.check_contraction(r["mu"], f["mu"], f["a_mu"], K, k, label + " mu")
    bad += HC.check_contraction(r["lv"], f["lv"], f["a_lv"], K, k, label + " lv")
    if c["eps"] is not None:
        s = HR.sample_ref(r["mu"], r["lv"], c["eps"])
        bad += HC.check_elementwise(r["sample"], s["sample"], s["a_sample"], k, label + " sample")
    g = HR.head_ref_g(c["d_mu"], c["d_lv"], c["d_s"], c["eps"], r["lv"], r["ldg"], lp=lp)
    if lp:
        bad += HC.check_bf16(r["g_lp"], g["g"], 2 * D, label + " g_lp")
        op = r["g_lp"].double()
    else:
        bad += HC.check_elementwise(r["g_ws"], g["g"][:, :2 * D], g["a_g"][:, :2 * D], k, label + " g_ws")
        op = r["g_ws"].double()
    b = HR.head_ref_bwd(op, c["h"], c["w_mu"], c["w_lv"], lp=lp)
    if r.get("dh") is not None:
        bad += HC.check_contraction(r["dh"], b["dh"], b["a_dh"], 2 * D, k, label + " dh")
    bad += HC.check_contraction(r["dW"], b["dW"], b["a_dW"], M, k, label + " dW")
    if r.get("db") is not None:
        src = {"g_lp": op, "g": g["g"]} if lp else {"g": op}  # rounded: the kernel's own g_lp; f32: the oracle's unrounded g
        want = HR.head_ref_bias(src, D, "rounded" if lp else "f32")
        bad += HC.check_bias(r["db"], want["db"], want["a_db"], k, label + " db")
    return bad


# (M, K, D, sample, ldt_extra, h_off) and the branches: forward through launch_proj when proj_eligible and D % 4 == 0 (gemm.hip:775)
# else the grouped generic engine (K = 200: K % 64 != 0; D = 6: D % 4 != 0); dh through launch_proj when ldt == ldg and
# proj_eligible (gemm.hip:856), the generic engine when ldt != ldg; dW through launch_wgrad when wgrad_eligible (gemm.hip:881),
# gemm_slow_kernel when h_lp sits 8 bytes off 16-byte alignment (wgrad_eligible and seg_fast_ok fail; gemm.hip:264-276; the
# forward then takes the slow kernel too).  The bf16 engine's fast mode-1 weight gradient is reached only past wgrad_eligible's
# 2^30-byte operand limit (K * ldg * 2 >= 2^30): not allocated here; the f32 head below covers mode 1.  Bias gradients: fused in
# reparam_bwd_pair_kernel<true> when 256 % (ldg / 8) == 0 (gemm.hip:827; D = 8, 32: ldg = 64), else colsum_kernel (D = 80, 96:
# ldg = 192).
HEAD_LP_CASES = [
    (37, 96, 16, True, 0, False),
    (2048, 512, 32, True, 0, False),     # the encoder heads (c2 / c3 K = 512)
    (4100, 256, 80, False, 0, False),    # decoder head, colsum_kernel bias
    (1000, 128, 96, True, 0, False),     # ldg = 192: colsum_kernel bias
    (300, 200, 8, True, 64, False),      # forward: grouped generic engine (K % 64); dh: generic engine (ldt != ldg)
    (513, 200, 6, False, 0, False),      # D % 4 != 0: generic forward
    (777, 256, 40, True, 0, True),       # h_lp 8 bytes off: gemm_slow_kernel forward and dW
    (40960, 256, 80, False, 0, False),   # decoder head at T B = 40960
]


@pytest.mark.parametrize("M,K,D,sample,ldt_extra,h_off", HEAD_LP_CASES)
def test_bf16_head_abi(hb, M, K, D, sample, ldt_extra, h_off):
    i = HC.head_inputs(M, K, D, M + K + D, sample)
    r = _head_lp_gpu(hb, i, ldt_extra, h_off)
    if sample:
        r["mu"], r["lv"] = r["mu_c"], r["lv_c"]
        assert torch.equal(r["mu_c"], r["out"][:, :D]) and torch.equal(r["lv_c"], r["out"][:, D:])
    else:
        r["mu"], r["lv"] = r["out"][:, :D], r["out"][:, D:]
    bad = _head_compare(i, r, "bf16", "bf16 head %s ldt+%d off=%d" % ((M, K, D), ldt_extra, h_off))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# f32 head through the ABI (fhvae_gauss_head_reparam_fwd / fhvae_gauss_head_bwd): forward a grouped launch of two problems
# (launch_gemm_group, gemm.hip:746-759), dh one two-segment contraction, dW one mode-1 (accumulating, auto split-K)
# contraction over the M rows (gemm.hip:949-969), bias colsum_kernel<float>.
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,D,sample", [(37, 96, 16, True), (2048, 512, 32, True), (2048, 1024, 32, True), (300, 200, 6, False),
                                          (81920, 256, 80, False)])
def test_f32_head_abi(hb, M, K, D, sample):
    lib = hb.load_library()
    i = HC.head_inputs(M, K, D, M + K + D + 1, sample)
    c = {k: (v.cuda() if v is not None else None) for k, v in i.items()}
    mu, lv = torch.empty(M, D, device="cuda"), torch.empty(M, D, device="cuda")
    smp = torch.empty(M, D, device="cuda") if sample else None
    assert lib.fhvae_gauss_head_reparam_fwd(_p(c["h"]), K, _p(c["w_mu"]), _p(c["w_lv"]), _p(c["b_mu"]), _p(c["b_lv"]), _p(c["eps"]),
                                            _p(mu), _p(lv), _p(smp), M, K, D, hb.F32, _st()) == 0
    g_ws = torch.empty(M, 2 * D, device="cuda")
    dh = torch.empty(M, K, device="cuda")
    dw = [torch.full((D, K), 0.125, device="cuda"), torch.full((D, K), -0.125, device="cuda")]
    db = [torch.full((D,), 0.5, device="cuda"), torch.full((D,), -0.25, device="cuda")]
    assert lib.fhvae_gauss_head_bwd(_p(c["h"]), K, _p(c["w_mu"]), _p(c["w_lv"]), _p(c["d_mu"]), _p(c["d_lv"]), _p(c["d_s"]), _p(c["eps"]),
                                    _p(lv), _p(g_ws), _p(dh), K, _p(dw[0]), _p(dw[1]), _p(db[0]), _p(db[1]), M, K, D, _st()) == 0
    torch.cuda.synchronize()
    r = {"mu": mu, "lv": lv, "sample": smp, "g_ws": g_ws, "dh": dh, "dW": torch.cat([dw[0] - 0.125, dw[1] + 0.125]),
         "db": torch.cat([db[0] - 0.5, db[1] + 0.25]), "ldg": 2 * D}
    bad = _head_compare(i, r, "f32", "f32 head %s" % ((M, K, D),))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# through the autograd binding
# ---------------------------------------------------------------------------------------------
def test_deferred_head_weight_gradients_match_the_oracle(hb):
    """With every parameter given a gradient sink, _GaussHeadLp queues its two weight-gradient contractions (_DEFER["extra"]) and
    flush_param_grads runs them in the grouped launch (fhvae_lstm_param_grads_multi).  Checked against the oracle chained on the
    kernel's own g_lp (fhvae_gauss_reparam_bwd_pair is deterministic: the same launch on the same inputs gives the same bits)."""
    M, K, D = 2048, 512, 32
    i = HC.head_inputs(M, K, D, 5)
    c = {k: v.cuda() for k, v in i.items()}
    ps = [c[k].clone() for k in ("w_mu", "b_mu", "w_lv", "b_lv")]
    for p in ps:
        p._fh_grad = torch.zeros_like(p)
        p.requires_grad_(True)
    h = c["h"].clone().requires_grad_(True)
    assert hb._DEFER["enabled"]
    mu, lv, smp = hb.gauss_head(h, *ps, c["eps"], h_lp=c["h"].bfloat16())
    ((mu * c["d_mu"]).sum() + (lv * c["d_lv"]).sum() + (smp * c["d_s"]).sum()).backward()
    assert len(hb._DEFER["extra"]) == 2
    hb.flush_param_grads()
    torch.cuda.synchronize()
    r = _head_lp_gpu(hb, i, want_db=False)
    assert torch.equal(r["out"][:, :D], mu) and torch.equal(r["out"][:, D:], lv)
    r.update(mu=mu, lv=lv, sample=smp, dh=h.grad, dW=torch.cat([ps[0]._fh_grad, ps[2]._fh_grad]),
             db=torch.cat([ps[1]._fh_grad, ps[3]._fh_grad]))
    bad = _head_compare(i, r, "bf16", "deferred bf16 head")
    assert not bad, bad


@pytest.mark.parametrize("T,B,K", [(20, 2048, 256), (40, 2048, 256)])
def test_decoder_head_and_lower_bound_end_to_end(hb, T, B, K):
    """The per-frame decoder head (no sample) + the lower bound at T B = 40960 and 81920, F = 80, through hip_binding.gauss_head and
    hip_binding.elbo: the head takes the lower bound's bf16 pair copy (PAIR_SIDE) and its bias gradients from the lower bound's
    partial rows (bias_from = "f32").  dh and dW are chained on the kernel's own pair rows, reproduced by one more
    fhvae_elbo_bwd on the same inputs (the rows are written by one lane each: deterministic)."""
    F = 80
    inp = HC.elbo_inputs(B, T, F, 32, 32, "typical", T + B)
    i = HC.head_inputs(T * B, K, F, T * B + 3, sample=False)
    c = {k: (v.cuda() if v is not None else None) for k, v in i.items()}
    x = inp["x"].transpose(0, 1).contiguous().cuda()
    z = [t.cuda() for t in inp["z"]]
    ns, glb = inp["num_segs"].cuda(), inp["ups"]["lower_bound"].cuda()
    h = c["h"].clone().requires_grad_(True)
    ps = [c[k].clone().requires_grad_(True) for k in ("w_mu", "b_mu", "w_lv", "b_lv")]
    used = hb.PAIR_SIDE["used"]
    x_mu, x_lv, _ = hb.gauss_head(h, *ps, None, h_lp=c["h"].bfloat16())
    lb = hb.elbo(x, x_mu, x_lv, *z, ns, (B, T, F, (F, B * F), (F, B * F)), False)[0]
    (lb * glb).sum().backward()
    torch.cuda.synchronize()
    assert hb.PAIR_SIDE["used"] == used + 1
    label = "e2e decoder T=%d B=%d" % (T, B)
    k = HC.HEAD["bf16"]
    f = HR.head_ref_fwd(c["h"], c["w_mu"], c["b_mu"], c["w_lv"], c["b_lv"], None, lp=True)
    bad = HC.check_contraction(x_mu, f["mu"], f["a_mu"], K, k, label + " mu")
    bad += HC.check_contraction(x_lv, f["lv"], f["a_lv"], K, k, label + " lv")
    bm = lambda t: t.detach().reshape(T, B, F).transpose(0, 1)
    args = (x.transpose(0, 1), bm(x_mu), bm(x_lv), *z, ns)
    wf = HR.elbo_ref_fwd(*args)
    bad += HC.check_elementwise(lb, wf["lower_bound"], wf["a_lower_bound"], HC.ELBO, label + " lower_bound")
    wb = HR.elbo_ref_bwd(*args, {"lower_bound": glb}, False)
    rep = {"x": inp["x"], "x_mu": bm(x_mu), "x_lv": bm(x_lv), "z": inp["z"]}
    _, gb, ex = _elbo_gpu(hb, rep, True, False, False, {"lower_bound": inp["ups"]["lower_bound"]}, inp["num_segs"], pair_ld=_pair_ld(F))
    bad += HC.check_elementwise(gb["d_x_lv"], wb["d_x_lv"], wb["a_d_x_lv"], HC.ELBO, label + " d_x_lv (replayed)")
    bad += HC.check_bf16(ex["pair"], _pair_ref(gb, _pair_ld(F)), 2 * F, label + " d_x_pair_lp (replayed)")
    b = HR.head_ref_bwd(ex["pair"].double(), c["h"], c["w_mu"], c["w_lv"], lp=True)
    bad += HC.check_contraction(h.grad, b["dh"], b["a_dh"], 2 * F, k, label + " dh")
    bad += HC.check_contraction(torch.cat([ps[0].grad, ps[2].grad]), b["dW"], b["a_dW"], T * B, k, label + " dW")
    s, a = HR.pair_colsum(wb["d_x_mu"], wb["d_x_lv"], wb["a_d_x_mu"], wb["a_d_x_lv"])
    bad += HC.check_bias(torch.cat([ps[1].grad, ps[3].grad]), s, a, k, label + " db (f32 source)")
    assert not bad, bad


@pytest.mark.parametrize("K", [512, 1024])
def test_encoder_heads_end_to_end(hb, K):
    """The z1 / z2 encoder heads at M = 2048, D = 32, K = sum(z1_hus) (512 at c2 / c3, 1024 at c4), through hip_binding.gauss_head
    (bf16 operands; no sinks: immediate weight gradients, fused bias sums since ldg = 64)."""
    M, D = 2048, 32
    i = HC.head_inputs(M, K, D, K + 9)
    c = {k: v.cuda() for k, v in i.items()}
    h = c["h"].clone().requires_grad_(True)
    ps = [c[k].clone().requires_grad_(True) for k in ("w_mu", "b_mu", "w_lv", "b_lv")]
    mu, lv, smp = hb.gauss_head(h, *ps, c["eps"], h_lp=c["h"].bfloat16())
    ((mu * c["d_mu"]).sum() + (lv * c["d_lv"]).sum() + (smp * c["d_s"]).sum()).backward()
    torch.cuda.synchronize()
    r = _head_lp_gpu(hb, i, want_db=False)  # the same launches: the kernel's own g_lp for the chained checks
    r.update(mu=mu, lv=lv, sample=smp, dh=h.grad, dW=torch.cat([ps[0].grad, ps[2].grad]), db=torch.cat([ps[1].grad, ps[3].grad]))
    bad = _head_compare(i, r, "bf16", "e2e encoder head K=%d" % K)
    assert not bad, bad


def test_mu2_gather_bwd(hb):
    """gather_bwd_kernel (loss.hip:75-83): scale != 1, a row-shard offset, targets outside the shard (skipped), heavy collisions
    (atomics), onto a non-zero table."""
    lib = hb.load_library()
    g = torch.Generator().manual_seed(2)
    S, D, B, off = 300, 32, 4096, 1000
    idx = torch.randint(off - 50, off + S + 50, (B,), generator=g)
    idx[:512] = off + 7
    idx[512:520] = off + S - 1
    idx[520:528] = off
    dm = torch.randn(B, D, generator=g)
    t0 = torch.randn(S, D, generator=g)
    dt = t0.cuda()
    assert lib.fhvae_mu2_gather_bwd(_p(dm.cuda()), _p(idx.cuda()), off, _p(dt), B, S, D, 0.37, _st()) == 0
    torch.cuda.synchronize()
    w = HR.mu2_gather_bwd_ref(dm.cuda(), idx.cuda(), off, S, 0.37, t0.cuda())
    k = HC.HEAD["f32"]
    bad = HC.check_bias(dt, w["dtable"], w["a_dtable"], k, "mu2_gather_bwd")
    assert not bad, bad
