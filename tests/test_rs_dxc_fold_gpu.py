"""d_xc computed inside the layer-0 launch of the partial-dh backward (csrc/lstm_bwd_rs.hip: f32 MFMAs on the register-held dgsum,
the waves summed through LDS and the members through the exchange buffer in fixed order, plain stores) against the same backward
with FHVAE_NO_DXC_FOLD=1 (the split-K f32 GEMM with atomics behind the launch) and the float64 oracle (oracle/lstm_lp_ref.py,
comparator and constants of tests/lstm_lp_compare.py).

B: the smallest batch for which the library reports the rows form at H = 256 (asked with fhvae_lstm_form), plus 16: a ragged last
cluster.  T = 2 (one exchange, the tail's parity is the never-used one) and 3; (I, Ic) = (80, 32) and (0, 64) (unit-major gates:
the configs' z1 encoder and decoder) and (80, 4) (one partly masked column tile; I + Ic no multiple of 8: the gates of the cluster
forward).  Ic = 136 and T = 1 keep the GEMM: there both runs are the same schedule and only the oracle is asked.

Bounds: the comparator's for every tensor of both runs; err_fold <= err_nofold + 2^-13 max|d_xc oracle| (max errors: the fold's
products are f32 MFMAs; the allowance is what a split-bf16 product would need: its dropped lo x lo term, 2^-16 of the sum of
absolute products, times 8 for cancellation -- measured: at most +0.0003 of the allowance, and the fold's maximum error at most
3.8 % of the comparator's bound); hn of the two runs bit-equal (the
forward is the same launch); the other gradients of the two runs within the comparator's noise floor (BF16["floor"] of scale) of
each other: dg is the same bits in both, what differs is the order of the f32 atomics of the weight- and bias-gradient sums, which
is the noise that floor was set above; two fold runs give the same d_xc bits."""
import ctypes as C
import os

import pytest
import torch

from lstm_lp_compare import BF16, compare, make_inputs, named_tensors
from oracle.lstm_lp_ref import lstm_lp_ref

pytestmark = pytest.mark.gpu

H, L = 256, 2


@pytest.fixture(scope="module")
def hb():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding

    hip_binding.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return hip_binding


@pytest.fixture(scope="module")
def rows_b(hb):
    """The smallest B (a multiple of 16) at which fhvae_lstm_form reports the rows form (1) for a bf16 two-layer H = 256 net."""
    lib = hb.load_library()
    x, xc, params, _, _ = make_inputs(16, 2, 80, 32, H, L, 1)
    ps = [p.cuda() for p in params]
    lp = torch.zeros(16, device="cuda", dtype=torch.uint8)  # (a host-only query: it asks whether the buffers are there, no more)
    for B in range(16, 4097, 16):
        d = hb.LstmDesc()
        hb._fill_lstm_desc(d, hb.BF16, (L, B, 2, 80, 32, H), x.cuda(), xc.cuda(), ps)
        d.lp = d.hs = d.pre = lp.data_ptr()
        if int(lib.fhvae_lstm_form(C.byref(d))) == 1:
            return B
    raise AssertionError("no batch up to 4096 takes the rows form")


def _run(hb, x, xc, T, params, g_out, g_hn, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ps = [p.cuda().requires_grad_(True) for p in params]
        xcd = xc.cuda().requires_grad_(True)
        hs_top, hn = hb.lstm_seq(x.cuda() if x is not None else None, xcd, T, ps, hb.BF16, top=2)
        form = dict(hb.LAST_LSTM_FORM)
        ((hn * g_hn.cuda()).sum() + (hs_top * g_out.cuda()).sum()).backward()
        hb.flush_param_grads()
        torch.cuda.synchronize()
        assert hb.lstm_sync_status() == 0, "a persistent recurrence launch gave up"
        assert form["form"] == 1 and form["layout"] >= 16, form
        return named_tensors(hs_top.detach().cpu(), hn.detach().cpu(), [p.grad.cpu() for p in ps], xcd.grad.cpu(), L)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _oracle(B, T, I, Ic):
    x, xc, params, g_out, g_hn = make_inputs(B, T, I, Ic, H, L, B + 7 * T + I + Ic)
    ref = lstm_lp_ref(x, xc, params, g_out, g_hn, T=T, rounding=True, partial_dh_bf16=True)
    return (x, xc, params, g_out, g_hn), named_tensors(ref["hs_top"], ref["hn"], ref["grads"], ref["d_xc"], L)


@pytest.mark.parametrize("T", [2, 3])
@pytest.mark.parametrize("I,Ic", [(80, 32), (0, 64), (80, 4)])
def test_fold_vs_gemm_vs_oracle(hb, rows_b, T, I, Ic):
    B = rows_b + 16
    label = "dxc B%d T%d I%d Ic%d" % (B, T, I, Ic)
    inp, want = _oracle(B, T, I, Ic)
    fold = _run(hb, *inp[:2], T, *inp[2:], {})
    again = _run(hb, *inp[:2], T, *inp[2:], {})
    gemm = _run(hb, *inp[:2], T, *inp[2:], {"FHVAE_NO_DXC_FOLD": "1"})
    bad = compare(fold, want, BF16, label + " fold") + compare(gemm, want, BF16, label + " gemm")
    scale = want["d_xc"].abs().max().item()
    e_fold = (fold["d_xc"].double() - want["d_xc"].double()).abs().max().item()
    e_gemm = (gemm["d_xc"].double() - want["d_xc"].double()).abs().max().item()
    print("%s d_xc max error: fold %.3e, gemm %.3e, allowance %.3e: (fold - gemm) / allowance = %.4f; fold share of the comparator's max bound %.4f" % (
        label, e_fold, e_gemm, 2.0 ** -13 * scale, (e_fold - e_gemm) / (2.0 ** -13 * scale), e_fold / scale / BF16["grad"]["max"]))
    if not e_fold <= e_gemm + 2.0 ** -13 * scale:
        bad.append("%s: d_xc error of the fold %.3e > %.3e + %.3e" % (label, e_fold, e_gemm, 2.0 ** -13 * scale))
    if not torch.equal(fold["d_xc"], again["d_xc"]):
        bad.append("%s: two fold runs differ in d_xc" % label)
    if not torch.equal(fold["hn"], gemm["hn"]) or not torch.equal(fold["hs_top"], gemm["hs_top"]):
        bad.append("%s: the forward outputs of the two runs differ" % label)
    for n, w in want.items():
        if n in ("hn", "hs_top", "d_xc"):
            continue
        diff = (fold[n].double() - gemm[n].double()).abs().max().item() / max(w.abs().max().item(), 1e-30)
        print("%s %-14s fold vs gemm run: max difference %.2e of scale" % (label, n, diff))
        if not diff <= BF16["floor"]:
            bad.append("%s %s: the two runs differ by %.3e of scale" % (label, n, diff))
    assert not bad, bad


@pytest.mark.parametrize("T,I,Ic", [(2, 80, 136), (1, 80, 32)])
def test_shapes_that_keep_the_gemm(hb, rows_b, T, I, Ic):
    """Ic > 64 and T = 1: lstm_plan leaves d_xc to the contraction behind the launch, switch or no switch."""
    B = rows_b + 16
    label = "dxc gemm-only B%d T%d I%d Ic%d" % (B, T, I, Ic)
    inp, want = _oracle(B, T, I, Ic)
    bad = []
    for env in ({}, {"FHVAE_NO_DXC_FOLD": "1"}):
        bad += compare(_run(hb, *inp[:2], T, *inp[2:], env), want, BF16, label + (" switch" if env else ""))
    assert not bad, bad
