"""One whole training step of fhvae.FHVAE -- forward, backward from each upstream of tests/step_compare.py, and the deferred
grouped weight-gradient flush -- against the composed float64 oracle of its own arithmetic (oracle/fhvae_step_ref.py), with one
comparator (tests/step_compare.py).  The per-kernel oracle tests pin each kernel; this file pins the glue of the bf16 model
that wires them together: top=0 / top=1 forwards, the `_fh_lp` twins and `_fh_head` shadows handed from a net to its head, the
sample of one head as the time-constant input of the next net, the three junctions where gradients are summed, and the flush.

The model runs the way training runs it: every parameter (and the table) has a gradient sink in hip_optim.FusedAdam's arena, so
the nets' and the heads' weight gradients are queued and come out of one grouped launch at hb.flush_param_grads().  Further
cases take the undeferred path, plain autograd gradients without sinks, and the module's own mu2_table parameter.  A wrapper
around hb.lstm_seq records the (form, layout, top) of each of the three nets; the oracle's schedule options of each net follow
from that (as test_lstm_lp_oracle_gpu._oracle_options), and each case asserts the schedules it was chosen for.  The
per-frame bf16 head must take the lower bound's ready-made pair rows (hb.PAIR_SIDE["used"]): the oracle gives it their f32 bias sums.
The oracle runs in float64 on the CPU.  Each case prints one STEPTABLE line per upstream and tensor group.

Measured on an MI355X (worst over the upstreams of the case; max / mean / signed of scale; every net took the schedule named):
  case (B, T, F, H, D, S)                 schedule  outputs               nets                  heads                 table
  ks    (64, 4, 80, 256, 32, 50)          ks        2.3e-4/8.9e-6/1.2e-6  1.8e-3/8.0e-5/5.4e-6  1.7e-3/3.0e-4/8.4e-5  6.4e-6/1.5e-7/1.0e-8
  ks, reference_compat                    ks        2.3e-4/8.9e-6/1.2e-6  1.6e-3/6.9e-5/1.1e-6  9.5e-4/9.6e-5/1.2e-5  6.5e-6/1.5e-7/1.0e-8
  T20   (64, 20, 80, 256, 32, 50)         ks        4.2e-4/4.0e-5/1.2e-5  2.4e-3/1.5e-4/6.4e-6  2.3e-3/4.9e-4/1.9e-4  2.2e-5/5.0e-7/3.8e-8
  rs    (1024, 3, 80, 256, 32, 300)       rs        3.8e-4/4.9e-6/1.2e-6  9.3e-4/4.8e-5/1.8e-6  6.5e-4/1.9e-4/3.4e-5  8.7e-7/3.7e-9/1.9e-10
  rows  (1500, 3, 80, 128, 32, 300)       rows      1.9e-4/1.8e-6/2.6e-7  5.9e-4/3.7e-5/2.4e-6  7.7e-4/1.6e-4/2.7e-5  4.3e-6/7.7e-9/3.8e-10
  cells (48, 5, 80, 64, 16, 40)           cells     3.5e-5/2.1e-6/1.5e-6  2.5e-3/5.2e-5/1.2e-5  1.2e-3/1.5e-4/5.3e-5  1.0e-5/2.2e-7/3.5e-8
  big   (256, 4, 80, 512, 32, 100)        big       1.8e-4/1.5e-5/9.5e-7  2.4e-3/1.3e-4/9.1e-6  2.5e-3/5.7e-4/1.6e-4  1.2e-6/2.9e-8/1.3e-9
  f32heads (48, 4, 6, 64, 4, 9)           cells     9.7e-6/1.2e-6/2.8e-7  6.6e-4/3.6e-6/4.5e-7  7.7e-6/2.6e-6/9.3e-7  2.3e-7/3.8e-8/1.1e-8
  ks, undeferred / no sinks / own table: the numbers of the ks row (same kernels, same order)
  f32 mode, ks shape                      cells     (see below)           1.2e-6/8.0e-8/5.0e-9  1.0e-6/3.3e-7/6.0e-8  9.0e-8/4.4e-9/1.2e-10
  f32 mode, cells shape                   cells     (see below)           7.4e-7/4.7e-8/6.6e-9  7.5e-7/1.8e-7/6.3e-8  1.2e-7/5.1e-9/5.0e-10
The heads' and the nets' bf16 numbers are those of the oracle's own noise floor (tests/step_compare.py, STEP_BF16), which is what
remains once every link is right.  f32 mode, outputs relative to max |oracle|: 2.6e-6/1.0e-6/5.0e-7, all of it neg_kld_z1 (a sum
near 0 of terms near 1: scale 0.1, terms 32); relative to the magnitude of the terms, as the test takes them, below 1e-8.
"""
import pytest
import torch

import step_compare as SC
from oracle.fhvae_step_ref import NETS, disc_mode_for, step_bwd, step_fwd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hb():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding

    hip_binding.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return hip_binding


def _sched(hb, form, layout, H):
    """The schedule name of test_lstm_lp_oracle_gpu for what fhvae_lstm_form / fhvae_lstm_layout_id returned."""
    if form == 0:
        return "big" if layout == 1 else "cells"
    if form == 2:
        return "ks"
    return "rs" if hb.lstm_kernel_names(1, H)[1] == "lstm_bwd_layer_rs_kernel" else "rows"


class _Step:
    """The model of one case on the GPU, and its gradients by state-dict name after a backward."""

    def __init__(self, hb, case, rc, dtype, sinks=True, own_table=False):
        from fhvae import FHVAE
        from hip_optim import FusedAdam

        B, T, F, H, D, S = case["shape"]
        self.hb, self.case, self.own_table = hb, case, own_table
        m = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, reference_compat=rc, compute_dtype=dtype,
                  num_seqs=S if own_table else None)
        m.load_state_dict(dict(case["sd"], mu2_table=case["table"].clone()) if own_table else case["sd"], strict=False)
        self.m = m.cuda()
        self.table = self.m.mu2_table if own_table else case["table"].cuda().requires_grad_(True)
        self.params = dict(self.m.named_parameters())
        self.params.pop("mu2_table", None)
        self.opt = FusedAdam(list(self.params.values()) + [self.table], lr=1e-3) if sinks else None
        self.x = case["x"].cuda()

    def run(self, upstream):
        from train_model import loss_function

        hb, c = self.hb, self.case
        if self.opt is not None:
            self.opt.zero_grad()
        else:
            for p in list(self.params.values()) + [self.table]:
                p.grad = None
        used = hb.PAIR_SIDE["used"]
        kw = {} if self.own_table else {"mu2_table": self.table}
        out = self.m(self.x, c["idx"], c["shape"][5], c["ns"], eps=c["eps"], **kw)
        obj = SC.objective(out, upstream) if isinstance(upstream, dict) else loss_function(out[0], out[1], float(upstream))
        obj.backward()
        hb.flush_param_grads()
        torch.cuda.synchronize()
        assert hb.lstm_sync_status() == 0, "a persistent recurrence launch gave up"
        grad = lambda p: None if p.grad is None else p.grad.detach().clone().cpu()
        return {"out": {n: o.detach().cpu() for n, o in zip(SC.OUT, out)}, "grads": {n: grad(p) for n, p in self.params.items()},
                "table": grad(self.table), "pair_side": hb.PAIR_SIDE["used"] - used}


def _check(hb, monkeypatch, cname, rc, dtype="bf16", ups=None, sinks=True, own_table=False, defer=True, label=None):
    spec = SC.GPU_CASES[cname]
    B, T, F, H, D, S = spec["shape"]
    bf = dtype == "bf16"
    label = label or "%s rc=%d %s" % (cname, rc, dtype)
    for k, v in spec.get("env", {}).items():
        monkeypatch.setenv(k, v)
    taken = []
    real = hb.lstm_seq

    def spy(x_tm, xc, T_, params, dtype=hb.F32, top=2, head=None):
        res = real(x_tm, xc, T_, params, dtype, top, head)
        taken.append((hb.LAST_LSTM_FORM["form"], hb.LAST_LSTM_FORM["layout"], top))
        return res

    monkeypatch.setattr(hb, "lstm_seq", spy)
    was = hb._DEFER["enabled"]
    hb.set_defer_param_grads(defer)
    try:
        case = SC.make_case(spec["shape"], 7)
        step = _Step(hb, case, rc, dtype, sinks, own_table)
        all_ups = SC.upstreams(B, rc)
        names = [u for u in (ups or spec["ups"] or list(all_ups)) if u in all_ups]
        ctx, bad, scheds, tops = None, [], None, None
        for uname in names:
            del taken[:]
            got = step.run(all_ups[uname])
            assert len(taken) == 3, taken  # the z2 net, the z1 net, the decoder, in this order (fhvae.py:160-165)
            sc = tuple(_sched(hb, f, l, H) for f, l, _ in taken)
            assert scheds in (None, sc)
            scheds, tops = sc, tuple(t for _, _, t in taken)
            lp_dec = bf and H % 8 == 0 and F % 8 == 0
            if ctx is None:  # (the per-frame bf16 head's bias sums default to "f32": the pair rows, checked below)
                ctx = step_fwd(case["sd"], case["x"], case["idx"], case["ns"], case["table"], case["eps"], rc, rounding=bf,
                               net_opts={n: SC.SCHED_OPTS[s] for n, s in zip(NETS, sc)}, disc_mode=disc_mode_for(B, S, D, bf))
            up = all_ups[uname]
            to_dec = not rc and (not isinstance(up, dict) or "lower_bound" in up or "log_px_z" in up)
            if lp_dec and to_dec and got["pair_side"] != 1:
                bad.append("%s %s: the per-frame head did not take the lower bound's pair rows" % (label, uname))
            want = step_bwd(ctx, all_ups[uname])
            want["out"] = ctx["out"]
            table = {}
            bad += SC.compare(got, want, SC.STEP_BF16 if bf else SC.STEP_F32, "%s %s" % (label, uname), table=table,
                               scales=None if bf else ctx["a_out"])
            SC.print_table("%s %s | %s tops %s" % (label, uname, "/".join(sc), tops), table)
        # the paths the case was chosen for
        if bf:
            if scheds != spec["sched"]:
                bad.append("%s: schedules %s, chosen for %s" % (label, scheds, spec["sched"]))
            want_tops = (0, 0, 1 if (H % 8 == 0 and F % 8 == 0) else 2)  # fhvae.py:160, 162, 164-165
            if tops != want_tops:
                bad.append("%s: tops %s, expected %s" % (label, tops, want_tops))
        assert not bad, bad
    finally:
        hb.set_defer_param_grads(was)


CASES = [(n, rc) for n, spec in SC.GPU_CASES.items() for rc in spec["rc"]]


@pytest.mark.parametrize("cname,rc", CASES)
def test_bf16_step_vs_composed_oracle(hb, monkeypatch, cname, rc):
    _check(hb, monkeypatch, cname, rc)


def test_undeferred_param_grads(hb, monkeypatch):
    """set_defer_param_grads(False): every weight gradient inside its own backward instead of at the grouped flush."""
    _check(hb, monkeypatch, "ks", False, ups=("loss", "log_px_z"), defer=False, label="nodefer ks")


def test_plain_autograd_gradients(hb, monkeypatch):
    """No gradient sinks: the Functions return their gradients to autograd (the path the older model tests take)."""
    _check(hb, monkeypatch, "ks", False, ups=("loss", "neg_kld_z1"), sinks=False, label="nosink ks")


def test_own_table_parameter(hb, monkeypatch):
    """The table as the module's own mu2_table parameter instead of the keyword."""
    _check(hb, monkeypatch, "ks", False, ups=("loss", "neg_kld_z2"), own_table=True, label="own-table ks")


@pytest.mark.parametrize("cname", ["ks", "cells"])
def test_f32_mode_vs_unrounded_oracle(hb, monkeypatch, cname):
    """compute_dtype="f32" (exact-f32 MFMA, f32 heads, top=2) against the rounding-off oracle under lstm_lp_compare.F32; the
    lower bound's outputs relative to the magnitude of their terms (step_compare.compare, `scales`)."""
    _check(hb, monkeypatch, cname, False, dtype="f32")
