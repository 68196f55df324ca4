"""Every schedule of the LSTM recurrence (hip_binding.lstm_seq) against the float64 oracle of its own arithmetic
(oracle/lstm_lp_ref.py: the bf16 rounding points of the kernels, or none in f32 mode), with one comparator and one set of constants
per mode (tests/lstm_lp_compare.py).  What is left between a kernel and its oracle is the f32 accumulation order and the one-ulp
flips of rb(h), rb(gate) or rb(dg) it causes now and then (the floor of the comparison, see tests/lstm_lp_compare.py): 4x to
100x below the differences from the f32 torch.nn.LSTM that test_ops_gpu / test_lstm_cluster_gpu bound.  Each case prints its measurements and, for comparison, the same numbers against
torch.nn.LSTM in f32."""
import os

import pytest
import torch

from lstm_lp_compare import BF16, F32, compare, make_inputs, measure, named_tensors
from oracle.lstm_lp_ref import lstm_lp_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hb():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding

    hip_binding.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return hip_binding


# the schedules: per-step cells (lstm.hip), large-tile cells (lstm_cell.hip), the persistent kernels (lstm_cluster.hip) in the
# contraction-split form ("ks"), the rows form with the dg exchange ("rows") and with the partial-dh backward ("rs",
# lstm_bwd_rs.hip; beside the register-stationary forward lstm_fwd_wr.hip where that applies)
def _schedule_ok(sched, form, layout):
    if sched == "cells":
        return form == 0 and layout == 0
    if sched == "big":
        return form == 0 and layout == 1
    return layout >= 16 and form == {"ks": 2, "rows": 1, "rs": 1}[sched]


def _oracle_options(sched):
    """The rounding-model options of each schedule (oracle/lstm_lp_ref.py cites the kernel lines)."""
    return {"rs": dict(partial_dh_bf16=True), "rows": {}, "ks": {},
            "cells": dict(bias_from_rounded_dg=True),
            "big": dict(bias_from_rounded_dg=True, dgsum_from_rounded_dg=True)}[sched]


def _run(hb, x, xc, T, params, g_out, g_hn, dtype, env=None, top=2, head=None):
    env = dict(env or {})
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ps = [p.cuda().requires_grad_(True) for p in params]
        xcd = xc.cuda().requires_grad_(True) if xc is not None else None
        hs_top, hn = hb.lstm_seq(x.cuda() if x is not None else None, xcd, T, ps, dtype, top=top,
                                 head=tuple(w.cuda() for w in head) if head is not None else None)
        form = dict(hb.LAST_LSTM_FORM)
        loss = (hn * g_hn.cuda()).sum()
        if top != 0:
            loss = loss + (hs_top * g_out.cuda()).sum()
        loss.backward()
        hb.flush_param_grads()
        torch.cuda.synchronize()
        assert hb.lstm_sync_status() == 0, "a persistent recurrence launch gave up"
        return {"form": form["form"], "layout": form["layout"], "hs_top": hs_top.detach().cpu() if top == 2 else None,
                "hs_lp": hs_top._fh_lp.cpu() if (top != 0 and dtype == hb.BF16) else None,
                "hn": hn.detach().cpu(), "grads": [p.grad.cpu() for p in ps],
                "d_xc": xcd.grad.cpu() if xcd is not None else None}
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _f32_lstm(x, xc, params, g_out, g_hn, L, H, top):
    """torch.nn.LSTM in f32 on the CPU: the yardstick of the older tests, measured here for comparison only."""
    T, B = g_out.shape[:2]
    I = x.shape[2] if x is not None else 0
    Ic = xc.shape[1] if xc is not None else 0
    lstm = torch.nn.LSTM(I + Ic, H, L)
    names = [n + "_l%d" % l for l in range(L) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    with torch.no_grad():
        for n, p in zip(names, params):
            getattr(lstm, n).copy_(p)
    xcl = xc.clone().requires_grad_(True) if Ic else None
    out, (hn, _) = lstm(torch.cat(([x] if I else []) + ([xcl[None].expand(T, B, Ic)] if Ic else []), -1))
    hn = torch.cat([hn[l] for l in range(L)], -1)
    loss = (hn * g_hn).sum() + ((out * g_out).sum() if top != 0 else 0)
    loss.backward()
    return named_tensors(out.detach() if top == 2 else None, hn.detach(), [getattr(lstm, n).grad for n in names],
                         xcl.grad if Ic else None, L)


def _summary(got, want):
    worst = {"max": 0.0, "mean": 0.0, "signed": 0.0}
    for n, w in want.items():
        if n in got and n != "hs_lp":
            st = measure(n, got[n], w)
            for k in worst:
                worst[k] = max(worst[k], st[k])
    return worst


def _check(hb, label, shape, sched, dtype="bf16", env=None, seed=0, w_scale=1.0, x_scale=1.0, top=2, head_dim=0):
    B, T, I, Ic, H, L = shape
    x, xc, params, g_out, g_hn = make_inputs(B, T, I, Ic, H, L, seed or (B + 7 * T + H + L), w_scale, x_scale)
    head = None
    if head_dim:
        g = torch.Generator().manual_seed(B + head_dim)
        head = (torch.randn(head_dim, L * H, generator=g) * 0.05, torch.randn(head_dim, L * H, generator=g) * 0.05)
    bf = dtype == "bf16"
    got = _run(hb, x, xc, T, params, g_out, g_hn, hb.BF16 if bf else hb.F32, env, top, head)
    assert _schedule_ok(sched, got["form"], got["layout"]), (label, sched, got["form"], got["layout"])
    opts = _oracle_options(sched) if bf else {}
    ref = lstm_lp_ref(x, xc, params, g_out if top != 0 else None, g_hn, T=T, rounding=bf, **opts)
    want = named_tensors(ref["hs_top"] if top == 2 else None, ref["hn"], ref["grads"], ref["d_xc"], L,
                         hs_lp=ref["hs_lp"] if (bf and top != 0) else None)
    have = named_tensors(got["hs_top"], got["hn"], got["grads"], got["d_xc"], L, hs_lp=got["hs_lp"])
    bad = compare(have, want, BF16 if bf else F32, label)
    o = _summary(have, want)
    f = _summary(have, _f32_lstm(x, xc, params, g_out, g_hn, L, H, top))
    print("LPTABLE | %s | %s form %d layout %d | %.2e %.2e %.2e | %.2e %.2e %.2e | %.0f %.0f" % (
        label, sched, got["form"], got["layout"], o["max"], o["mean"], o["signed"], f["max"], f["mean"], f["signed"],
        f["max"] / max(o["max"], 1e-30), f["mean"] / max(o["mean"], 1e-30)))
    assert not bad, bad
    return got


# (B, T, I, Ic, H, L), schedule.  The shapes of test_lstm_cluster_gpu.CASES: whole tiles, ragged clusters, batches smaller than
# the cluster count, one layer, H = 128, more rows than one launch covers, T = 1, a time-constant input with and without a
# per-frame one
CASES = [((256, 20, 80, 0, 256, 2), "ks"), ((100, 7, 80, 32, 256, 2), "ks"), ((16, 5, 0, 64, 256, 2), "ks"),
         ((5, 3, 80, 0, 256, 2), "ks"), ((2048, 20, 80, 0, 256, 2), "rs"), ((300, 6, 40, 0, 128, 2), "ks"),
         ((64, 4, 80, 0, 256, 1), "ks"), ((2500, 3, 80, 32, 256, 2), "rs"), ((700, 1, 80, 0, 256, 2), "rs"),
         ((1000, 9, 0, 64, 128, 1), "ks"), ((1024, 5, 80, 0, 256, 2), "rs"), ((1500, 4, 80, 32, 128, 2), "rows"),
         ((4100, 2, 0, 64, 256, 1), "rs"), ((2048, 3, 80, 32, 256, 2), "rs"), ((1024, 4, 0, 64, 256, 2), "rs"),
         # test_partial_dh_backward_vs_dg_exchange: ragged clusters with a time-constant input, more than one launch
         ((1100, 4, 80, 32, 256, 2), "rs"), ((3000, 3, 80, 0, 256, 2), "rs"),
         # test_lstm_seq_vs_torch_lstm (bf16): tiny and odd H on the per-step cells
         ((5, 4, 8, 8, 8, 2), "cells"), ((70, 20, 80, 0, 64, 2), "cells"), ((33, 20, 80, 32, 48, 2), "cells"),
         ((64, 20, 0, 64, 256, 2), "ks"), ((300, 20, 80, 32, 256, 2), "ks"),
         # three layers (per-step cells), T = 40, the large-tile cells by default (H = 512, B = 2048)
         ((256, 6, 80, 0, 256, 3), "cells"), ((512, 40, 80, 0, 128, 2), "ks"), ((2048, 3, 80, 32, 512, 2), "big")]


@pytest.mark.parametrize("shape,sched", CASES)
def test_schedule_vs_rounding_oracle(hb, shape, sched):
    _check(hb, "B%d T%d I%d Ic%d H%d L%d" % shape, shape, sched)


# every FHVAE_* switch of test_lstm_cluster_gpu.SWITCHES at its shape, against the oracle of the schedule it selects
SWITCHES = [("FHVAE_NO_CLUSTER", "1", (1024, 4, 80, 32, 256, 2), "cells"),
            ("FHVAE_NO_RS", "1", (1024, 4, 80, 32, 256, 2), "rows"),
            ("FHVAE_NO_FWD_WR", "1", (1024, 4, 80, 32, 256, 2), "rs"),
            ("FHVAE_NO_FOLD", "1", (1024, 4, 80, 32, 256, 2), "rs"),
            ("FHVAE_NO_XC_FOLD", "1", (1024, 4, 0, 64, 256, 2), "rs"),
            ("FHVAE_NO_WGRAD", "1", (1024, 4, 80, 32, 256, 2), "rs"),
            ("FHVAE_CLUSTER_TLOG", "1", (1024, 4, 80, 32, 256, 2), "rs"),
            ("FHVAE_BIG_CELLS", "1", (256, 4, 80, 32, 512, 2), "big"),
            ("FHVAE_BIG_CELLS", "0", (2048, 3, 80, 32, 512, 2), "cells"),
            ("FHVAE_NO_CLUSTER", "1", (256, 20, 80, 0, 256, 2), "cells"),
            ("FHVAE_NO_FOLD", "1", (256, 5, 80, 32, 256, 2), "ks")]


@pytest.mark.parametrize("name,value,shape,sched", SWITCHES)
def test_switch_vs_rounding_oracle(hb, name, value, shape, sched):
    _check(hb, "%s=%s B%d T%d I%d Ic%d H%d L%d" % ((name, value) + shape), shape, sched, env={name: value})


# saturated gates and a growing cell state (input weights and biases x4, inputs x3, T = 40): the fast tanhf_ / sigmoidf_ forms
# (lstm_point.h) in their tails and the dc carry where training takes it.  W_hh keeps its scale: scaled x4 as well, the recurrence
# stops damping the one-ulp flips of rb(h) (measured: gradient mean errors 2e-4 .. 6e-4 of scale on every schedule, the oracle
# against itself with f32-level noise alike), and the comparison would measure that chaos instead of the kernels
@pytest.mark.parametrize("shape,sched", [((1024, 40, 80, 0, 256, 2), "rs"), ((256, 40, 80, 32, 256, 2), "ks"),
                                         ((1500, 40, 80, 0, 128, 2), "rows"), ((128, 40, 80, 32, 64, 2), "cells")])
def test_saturated_vs_rounding_oracle(hb, shape, sched):
    _check(hb, "sat B%d T%d I%d Ic%d H%d L%d" % shape, shape, sched, w_scale=4.0, x_scale=3.0)


@pytest.mark.parametrize("shape,sched", [((2048, 6, 0, 32, 256, 2), "rs"), ((256, 6, 0, 32, 256, 2), "ks"),
                                         ((192, 6, 0, 32, 64, 2), "cells")])
def test_decoder_mode_top1(hb, shape, sched):
    """top=1 (the decoder, fhvae.py): the data is the bf16 twin hs_top._fh_lp = rb(h), bit-equal to the bf16 cast of a top=2 run
    on the same inputs; hn and every gradient against the oracle."""
    B, T, I, Ic, H, L = shape
    label = "top1 B%d T%d I%d Ic%d H%d L%d" % shape
    got = _check(hb, label, shape, sched, top=1)
    x, xc, params, g_out, g_hn = make_inputs(B, T, I, Ic, H, L, B + 7 * T + H + L)
    two = _run(hb, x, xc, T, params, g_out, g_hn, hb.BF16, top=2)
    assert torch.equal(got["hs_lp"], two["hs_top"].to(torch.bfloat16))


@pytest.mark.parametrize("shape,sched,Dh", [((2048, 5, 80, 0, 256, 2), "rs", 32), ((256, 5, 80, 0, 256, 2), "ks", 32),
                                            ((192, 5, 80, 0, 128, 1), "ks", 80), ((2048, 5, 80, 0, 128, 2), "rows", 32),
                                            ((192, 5, 80, 0, 64, 1), "cells", 80)])
def test_encoder_mode_top0_head(hb, shape, sched, Dh):
    """top=0 with the Gaussian head behind the net (the encoders): hn and every gradient against the oracle."""
    _check(hb, "top0 B%d T%d I%d Ic%d H%d L%d" % shape, shape, sched, top=0, head_dim=Dh)


def test_undeferred_param_grads(hb):
    """The parameter gradients computed inside the backward (set_defer_param_grads(False)) instead of at the flush."""
    was = hb._DEFER["enabled"]
    hb.set_defer_param_grads(False)
    try:
        _check(hb, "nodefer B1024 T5", (1024, 5, 80, 32, 256, 2), "rs")
        _check(hb, "nodefer B256 T5", (256, 5, 80, 32, 256, 2), "ks")
    finally:
        hb.set_defer_param_grads(was)


@pytest.mark.parametrize("shape,sched,env", [((5, 4, 6, 0, 8, 2), "cells", {}), ((5, 4, 6, 4, 8, 2), "cells", {}),
                                             ((7, 3, 0, 8, 16, 1), "cells", {}), ((70, 20, 80, 0, 64, 2), "cells", {}),
                                             ((33, 20, 80, 32, 48, 2), "cells", {}), ((64, 20, 0, 64, 256, 2), "cells", {}),
                                             ((300, 20, 80, 32, 256, 2), "cells", {}),
                                             ((256, 4, 80, 32, 512, 2), "big", {"FHVAE_BIG_CELLS": "1"}),
                                             ((2048, 3, 80, 0, 512, 2), "big", {})])
def test_f32_mode_vs_float64(hb, shape, sched, env):
    _check(hb, "f32 B%d T%d I%d Ic%d H%d L%d" % shape, shape, sched, dtype="f32", env=env)
