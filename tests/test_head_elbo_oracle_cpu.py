"""The float64 oracle of the heads and the lower bound (oracle/head_elbo_ref.py) and the comparator of the GPU checks
(tests/head_elbo_compare.py), on the CPU: with rounding off the oracle is ref_cpu.elbo_terms, ref_cpu.gauss_sample and float64
autograd; the oracle against itself, its inputs moved by one f32 ulp, stays under the constants; and with those constants the
comparator rejects every deliberately wrong variant in the oracle's `_fault` list, at the model's shapes."""
import pytest
import torch

import head_elbo_compare as HC
from oracle import head_elbo_ref as HR
from oracle import ref_cpu as R

NAMES = ("lower_bound", "log_px_z", "neg_kld_z1", "neg_kld_z2", "log_pmu2")
GRADS = ("d_z1_mu", "d_z1_lv", "d_z2_mu", "d_z2_lv", "d_mu2")


def _close(got, want, what):
    tol = 1e-10 * max(1.0, want.abs().max().item())
    assert (got - want).abs().max().item() <= tol, (what, (got - want).abs().max().item())


@pytest.mark.parametrize("detach", [True, False])
@pytest.mark.parametrize("scalar", [False, True])
@pytest.mark.parametrize("regime", ["typical", "lv_neg", "prior"])
def test_elbo_oracle_is_elbo_terms_f64(detach, scalar, regime):
    B, T, F, D1, D2 = 9, 5, 12, 8, 65
    inp = HC.elbo_inputs(B, T, F, D1, D2, regime, 7)
    x, xm, xl = (inp[k].double() for k in ("x", "x_mu", "x_lv"))
    xm.requires_grad_(True), xl.requires_grad_(True)
    z = [t.double().requires_grad_(True) for t in inp["z"]]
    ns = 17 if scalar else inp["num_segs"]
    outs = R.elbo_terms(x, xm, xl, *z, ns if scalar else ns.double(), reference_detach=detach)
    want = HR.elbo_ref_fwd(x, xm, xl, *z, ns)
    for n, o in zip(NAMES, outs):
        _close(want[n], o.detach(), n)
    ups = {k: v.double() for k, v in inp["ups"].items()}
    sum((o * ups[n]).sum() for n, o in zip(NAMES, outs) if o.requires_grad).backward()
    # the kernels take the upstream gradients of the detached outputs as given and drop their paths (loss.hip:193, 203)
    got = HR.elbo_ref_bwd(x, xm, xl, *z, ns, ups, detach)
    for n, t in zip(GRADS, z):
        _close(got[n], t.grad, n)
    if detach:
        assert got["d_x_mu"] is None and xm.grad is None
    else:
        _close(got["d_x_mu"], xm.grad, "d_x_mu")
        _close(got["d_x_lv"], xl.grad, "d_x_lv")


def test_elbo_oracle_takes_absent_upstreams_as_zero():
    inp = HC.elbo_inputs(4, 3, 8, 8, 8, "typical", 1)
    args = (inp["x"], inp["x_mu"], inp["x_lv"], *inp["z"], inp["num_segs"])
    for k in HR.UPSTREAMS:
        only = {k: inp["ups"][k]}
        zeros = {n: (inp["ups"][n] if n == k else torch.zeros(4)) for n in HR.UPSTREAMS}
        a, b = HR.elbo_ref_bwd(*args, only, False), HR.elbo_ref_bwd(*args, zeros, False)
        for n in GRADS + ("d_x_mu", "d_x_lv"):
            assert torch.equal(a[n], b[n]), (k, n)


@pytest.mark.parametrize("sample", [True, False])
def test_f32_head_oracle_is_autograd_f64(sample):
    M, K, D = 37, 96, 16
    i = HC.head_inputs(M, K, D, 3, sample)
    h, wm, bm, wl, bl = (i[k].double().requires_grad_(True) for k in ("h", "w_mu", "b_mu", "w_lv", "b_lv"))
    mu, lv = torch.nn.functional.linear(h, wm, bm), torch.nn.functional.linear(h, wl, bl)
    tot = (mu * i["d_mu"].double()).sum() + (lv * i["d_lv"].double()).sum()
    if sample:
        smp = R.gauss_sample(mu, lv, i["eps"].double())
        tot = tot + (smp * i["d_s"].double()).sum()
    tot.backward()
    f = HR.head_ref_fwd(h, wm, bm, wl, bl, i["eps"], lp=False)
    _close(f["mu"], mu.detach(), "mu")
    _close(f["lv"], lv.detach(), "lv")
    if sample:
        _close(f["sample"], smp.detach(), "sample")
    g = HR.head_ref_g(i["d_mu"], i["d_lv"], i["d_s"], i["eps"], f["lv"], 2 * D + 8, lp=False)
    assert torch.all(g["g"][:, 2 * D:] == 0)
    b = HR.head_ref_bwd(g["g"], h, wm, wl, lp=False)
    _close(b["dh"], h.grad, "dh")
    _close(b["dW"][:D], wm.grad, "dW_mu")
    _close(b["dW"][D:], wl.grad, "dW_lv")
    db = HR.head_ref_bias(g, D, "f32")["db"]
    _close(db[:D], bm.grad, "db_mu")
    _close(db[D:], bl.grad, "db_lv")


def test_bf16_head_oracle_rounds_the_operands_and_g():
    """The bf16 form is the f32 form of rb(h), rb(W) and rb(g); the rounding is f2bf's (round to nearest even from f32)."""
    M, K, D = 70, 64, 8
    i = HC.head_inputs(M, K, D, 4)
    rbf = lambda t: t.bfloat16().double()
    f = HR.head_ref_fwd(i["h"], i["w_mu"], i["b_mu"], i["w_lv"], i["b_lv"], i["eps"], lp=True)
    f0 = HR.head_ref_fwd(rbf(i["h"]), rbf(i["w_mu"]), i["b_mu"], rbf(i["w_lv"]), i["b_lv"], i["eps"], lp=False)
    assert torch.equal(f["mu"], f0["mu"]) and torch.equal(f["sample"], f0["sample"])
    g = HR.head_ref_g(i["d_mu"], i["d_lv"], i["d_s"], i["eps"], f["lv"], 64, lp=True)
    assert torch.equal(g["g_lp"], rbf(g["g"].float()))
    b = HR.head_ref_bwd(g["g_lp"], i["h"], i["w_mu"], i["w_lv"], lp=True)
    assert torch.allclose(b["dh"], g["g_lp"][:, :2 * D] @ torch.cat([rbf(i["w_mu"]), rbf(i["w_lv"])]), rtol=1e-13, atol=0)
    assert torch.allclose(b["dW"], g["g_lp"][:, :2 * D].T @ rbf(i["h"]), rtol=1e-13, atol=0)


def test_pair_rows_and_colsum_model_the_pair_kernel():
    B, T, F = 5, 3, 8
    dm, dl = torch.randn(B, T, F).double(), torch.randn(B, T, F).double()
    p = HR.pair_rows(dm, dl, 2 * F + 16)
    for t in range(T):
        for b in range(B):
            r = p[t * B + b]
            assert torch.equal(r[:F], HR.rb(dm[b, t])) and torch.equal(r[F:2 * F], HR.rb(dl[b, t])) and not r[2 * F:].any()
    s, a = HR.pair_colsum(dm, dl)
    assert torch.allclose(s, torch.cat([dm.sum((0, 1)), dl.sum((0, 1))]), rtol=1e-14, atol=1e-14)
    assert torch.all(a >= s.abs())


def test_mu2_gather_bwd_oracle():
    S, D, B = 10, 4, 50
    g = torch.Generator().manual_seed(0)
    dm = torch.randn(B, D, generator=g)
    idx = torch.randint(-3, 2 * S, (B,), generator=g)
    t0 = torch.randn(S, D, generator=g)
    got = HR.mu2_gather_bwd_ref(dm, idx, 5, S, 0.37, t0)["dtable"]
    want = t0.double().clone()
    sc = float(torch.tensor(0.37, dtype=torch.float32))
    for b in range(B):
        s = int(idx[b]) - 5
        if 0 <= s < S:
            want[s] += sc * dm[b].double()
    _close(got, want, "dtable")


# ---------------------------------------------------------------------------------------------
# the noise floor and the rejected faults, at the model's shapes
# ---------------------------------------------------------------------------------------------
def _ulp(x: torch.Tensor, seed: int) -> torch.Tensor:
    """x with a random half of its entries moved by one f32 ulp (either way)."""
    g = torch.Generator().manual_seed(seed)
    x = x.float()
    m = torch.rand(x.shape, generator=g) < 0.5
    up = torch.rand(x.shape, generator=g) < 0.5
    y = torch.where(up, torch.nextafter(x, torch.full_like(x, float("inf"))), torch.nextafter(x, torch.full_like(x, -float("inf"))))
    return torch.where(m, y, x)


def _elbo_checks(got_f, got_b, want_f, want_b, B, T, F, quiet=True, log=None, pair=None):
    bad = []
    for n in NAMES:
        bad += HC.check_elementwise(got_f[n], want_f[n], want_f["a_" + n], HC.ELBO, "elbo " + n, quiet, log, (("row", torch.arange(B)),))
    for n in GRADS:
        bad += HC.check_elementwise(got_b[n], want_b[n], want_b["a_" + n], HC.ELBO, "elbo " + n, quiet, log)
    if want_b["d_x_mu"] is not None:
        for n in ("d_x_mu", "d_x_lv"):
            bad += HC.check_elementwise(got_b[n], want_b[n], want_b["a_" + n], HC.ELBO, "elbo " + n, quiet, log, HC.row_time_bins(B, T, F))
    return bad


@pytest.fixture(scope="module")
def model_elbo():
    """The decoder's lower bound at c2's shape (B = 2048, T = 20, F = 80, D1 = D2 = 32), typical regime."""
    B, T, F = 2048, 20, 80
    inp = HC.elbo_inputs(B, T, F, 32, 32, "typical", 11)
    args = (inp["x"], inp["x_mu"], inp["x_lv"], *inp["z"], inp["num_segs"])
    return B, T, F, inp, args, HR.elbo_ref_fwd(*args), HR.elbo_ref_bwd(*args, inp["ups"], False)


@pytest.fixture(scope="module")
def model_head():
    """The decoder head at c2's shape (M = T B = 40960, K = 256, D = F = 80), bf16 operands."""
    M, K, D = 40960, 256, 80
    i = HC.head_inputs(M, K, D, 12, sample=True)
    f = HR.head_ref_fwd(i["h"], i["w_mu"], i["b_mu"], i["w_lv"], i["b_lv"], i["eps"], lp=True)
    g = HR.head_ref_g(i["d_mu"], i["d_lv"], i["d_s"], i["eps"], f["lv"], 192, lp=True)
    b = HR.head_ref_bwd(g["g_lp"], i["h"], i["w_mu"], i["w_lv"], lp=True)
    return M, K, D, i, f, g, b


def test_noise_floor_is_below_the_constants(model_elbo, model_head):
    """The oracle against itself with the f32 inputs moved by one ulp.  In the bf16 form the operands h, W and the chained g_lp
    stay those of the unmoved inputs (a one-ulp move flips a bf16 rounding now and then: a 2^-8 step of the form's own
    resolution, not f32 noise).  Every statistic must stay below half its constant."""
    log = []
    B, T, F, inp, args, wf, wb = model_elbo
    for regime, seed in (("typical", 11), ("lv_neg", 12), ("lv_pos", 13), ("prior", 14)):
        if regime != "typical":
            inp = HC.elbo_inputs(512, T, F, 32, 32, regime, seed)
            args = (inp["x"], inp["x_mu"], inp["x_lv"], *inp["z"], inp["num_segs"])
            wf, wb = HR.elbo_ref_fwd(*args), HR.elbo_ref_bwd(*args, inp["ups"], False)
        pa = [_ulp(t, 1 + k) for k, t in enumerate(args[:-1])] + [args[-1]]
        ups = {k: _ulp(v, 20 + j) for j, (k, v) in enumerate(inp["ups"].items())}
        nb = pa[0].shape[0]
        assert not _elbo_checks(HR.elbo_ref_fwd(*pa), HR.elbo_ref_bwd(*pa, ups, False), wf, wb, nb, T, F, log=log)
        s0, a0 = HR.pair_colsum(wb["d_x_mu"], wb["d_x_lv"], wb["a_d_x_mu"], wb["a_d_x_lv"])
        pb = HR.elbo_ref_bwd(*pa, ups, False)
        s1, _ = HR.pair_colsum(pb["d_x_mu"], pb["d_x_lv"])
        assert not HC.check_bias(s1, s0, a0, HC.HEAD["bf16"], "colsum " + regime, True, log)
    M, K, D, i, f, g, b = model_head
    for mode in ("bf16", "f32"):
        k = HC.HEAD[mode]
        lp = mode == "bf16"
        hp = i["h"] if lp else _ulp(i["h"], 31)
        wm, wl = (i["w_mu"], i["w_lv"]) if lp else (_ulp(i["w_mu"], 32), _ulp(i["w_lv"], 33))
        f1 = HR.head_ref_fwd(hp, wm, _ulp(i["b_mu"], 34), wl, _ulp(i["b_lv"], 35), _ulp(i["eps"], 36), lp=lp)
        f0 = f if lp else HR.head_ref_fwd(i["h"], i["w_mu"], i["b_mu"], i["w_lv"], i["b_lv"], i["eps"], lp=False)
        bad = HC.check_contraction(f1["mu"], f0["mu"], f0["a_mu"], K, k, mode + " mu", True, log)
        bad += HC.check_contraction(f1["lv"], f0["lv"], f0["a_lv"], K, k, mode + " lv", True, log)
        s1 = HR.sample_ref(_ulp(f0["mu"], 37), _ulp(f0["lv"], 38), _ulp(i["eps"], 39))
        s0 = HR.sample_ref(f0["mu"], f0["lv"], i["eps"])
        bad += HC.check_elementwise(s1["sample"], s0["sample"], s0["a_sample"], k, mode + " sample", True, log)
        g0 = g if lp else HR.head_ref_g(i["d_mu"], i["d_lv"], i["d_s"], i["eps"], f0["lv"], 2 * D, lp=False)
        g1 = HR.head_ref_g(_ulp(i["d_mu"], 40), _ulp(i["d_lv"], 41), _ulp(i["d_s"], 42), i["eps"], f0["lv"], g0["g"].shape[1], lp=lp)
        op0 = g0["g_lp"] if lp else g0["g"]
        op1 = g0["g_lp"] if lp else g1["g"]
        b0 = b if lp else HR.head_ref_bwd(op0, i["h"], i["w_mu"], i["w_lv"], lp=False)
        b1 = HR.head_ref_bwd(op1, hp, wm, wl, lp=lp)
        bad += HC.check_contraction(b1["dh"], b0["dh"], b0["a_dh"], 2 * D, k, mode + " dh", True, log)
        bad += HC.check_contraction(b1["dW"], b0["dW"], b0["a_dW"], M, k, mode + " dW", True, log)
        for src in (("rounded", "f32") if lp else ("f32",)):
            d0, d1 = HR.head_ref_bias(g0, D, src), HR.head_ref_bias(g1 if src == "f32" else g0, D, src)
            bad += HC.check_bias(d1["db"], d0["db"], d0["a_db"], k, "%s db (%s)" % (mode, src), True, log)
        assert not bad, bad
    for label, st in log:
        print(label, st if "max" not in st else HC.fmt(st))
    for label, st in log:
        if "max" not in st:
            continue
        mode = "bf16" if label.startswith("bf16") or label.startswith("colsum") else "f32"
        if label.startswith("elbo"):
            lim = HC.ELBO["max"]
        elif " db" in label or label.startswith("colsum"):
            lim = HC.HEAD[mode]["bmax"]
        elif "sample" in label:
            lim = HC.HEAD[mode]["emax"]
        else:
            lim = HC.HEAD[mode]["cmax"]
        assert st["max"] <= 0.5 * lim, (label, st["max"], lim)


def _rejects(bad):
    assert bad, "the comparator accepted a faulted oracle"


@pytest.mark.parametrize("fault", [{"drop_step": (1000, 7)}, {"scalar_nsegs": 100}, {"lv_no_half": True}])
def test_rejects_elbo_faults(model_elbo, fault):
    B, T, F, inp, args, wf, wb = model_elbo
    bf = HR.elbo_ref_bwd(*args, inp["ups"], False, _fault=fault)
    ff = HR.elbo_ref_fwd(*args, _fault=fault)
    _rejects(_elbo_checks(ff, bf, wf, wb, B, T, F))


def test_rejects_the_prior_term_under_detach(model_elbo):
    B, T, F, inp, args, wf, wb = model_elbo
    w = HR.elbo_ref_bwd(*args, inp["ups"], True)
    got = HR.elbo_ref_bwd(*args, inp["ups"], True, _fault={"prior_kept": True})
    _rejects(HC.check_elementwise(got["d_mu2"], w["d_mu2"], w["a_d_mu2"], HC.ELBO, quiet=True))


def test_rejects_colsum_without_the_last_odd_segment():
    B, T, F = 2047, 20, 80
    inp = HC.elbo_inputs(B, T, F, 32, 32, "typical", 5)
    w = HR.elbo_ref_bwd(inp["x"], inp["x_mu"], inp["x_lv"], *inp["z"], inp["num_segs"], inp["ups"], False)
    s, a = HR.pair_colsum(w["d_x_mu"], w["d_x_lv"], w["a_d_x_mu"], w["a_d_x_lv"])
    s1, _ = HR.pair_colsum(w["d_x_mu"], w["d_x_lv"], _fault={"drop_last_b": True})
    _rejects(HC.check_bias(s1, s, a, HC.HEAD["bf16"], quiet=True))


@pytest.mark.parametrize("fault", [{"pad_nonzero": True}, {"batch_major": True}])
def test_rejects_pair_row_faults(model_elbo, fault):
    B, T, F, inp, args, wf, wb = model_elbo
    want = HR.pair_rows(wb["d_x_mu"], wb["d_x_lv"], 192)
    want_u = torch.zeros_like(want)
    want_u[:, :2 * F] = torch.cat([wb["d_x_mu"], wb["d_x_lv"]], 2).transpose(0, 1).reshape(T * B, 2 * F)
    got = HR.pair_rows(wb["d_x_mu"], wb["d_x_lv"], 192, _fault=fault).to(torch.bfloat16)
    assert not HC.check_bf16(HR.pair_rows(wb["d_x_mu"], wb["d_x_lv"], 192).to(torch.bfloat16), want_u, 2 * F, quiet=True)
    _rejects(HC.check_bf16(got, want_u, 2 * F, quiet=True))


@pytest.mark.parametrize("fault", [{"drop_k_tile": True}, {"drop_m_tile": True}])
def test_rejects_head_contraction_faults(model_head, fault):
    M, K, D, i, f, g, b = model_head
    got = HR.head_ref_bwd(g["g_lp"], i["h"], i["w_mu"], i["w_lv"], lp=True, _fault=fault)
    k = HC.HEAD["bf16"]
    bad = HC.check_contraction(got["dh"], b["dh"], b["a_dh"], 2 * D, k, quiet=True)
    bad += HC.check_contraction(got["dW"], b["dW"], b["a_dW"], M, k, quiet=True)
    _rejects(bad)


@pytest.mark.parametrize("got_from,want_from", [("f32", "rounded"), ("rounded", "f32")])
def test_rejects_bias_from_the_wrong_source(model_head, got_from, want_from):
    M, K, D, i, f, g, b = model_head
    got, want = HR.head_ref_bias(g, D, got_from), HR.head_ref_bias(g, D, want_from)
    _rejects(HC.check_bias(got["db"], want["db"], want["a_db"], HC.HEAD["bf16"], quiet=True))


def test_rejects_exp_lv_in_the_sample(model_head):
    M, K, D, i, f, g, b = model_head
    got = HR.sample_ref(f["mu"], f["lv"], i["eps"], _fault={"exp_full_lv": True})
    _rejects(HC.check_elementwise(got["sample"], f["sample"], f["a_sample"], HC.HEAD["bf16"], quiet=True))
