"""One comparator for a whole training step of fhvae.FHVAE against the composed float64 oracle (oracle/fhvae_step_ref.py): the
case tables, the set of upstreams and one comparison routine, shared by tests/test_step_oracle_gpu.py (the model on the GPU)
and tests/test_step_oracle_cpu.py (the oracle against float64 autograd, its own noise floor, and the faults it must reject).

Every tensor goes through lstm_lp_compare.measure / failures with lstm_lp_compare.BF16 / F32: the same four measures (max,
mean, signed, local) and the same bins for the LSTM tensors; head weights are binned as (64, 64), head biases and the six
outputs as (64,), the table as (32, 64) (lstm_lp_compare.bin_divisors by the parameter's own name).  The constants are lstm_lp_compare's
except where the floor measurement (test_step_oracle_cpu.test_floor) forced one up: see STEP_BF16.
"""
import copy

import torch

from lstm_lp_compare import BF16, F32, failures, fmt, measure
from oracle import ref_cpu as R
from oracle.fhvae_step_ref import NETS, OUT

ALPHA = 10.0

# (B, T, F, H, D, S): two layers per net.  The smallest shapes at which each path still runs (tests/test_step_oracle_gpu.py
# asserts the schedule of every net: "sched", for the z2 net, the z1 net and the decoder); "ups": the upstreams of the case (None: all), "rc": the reference_compat values
GPU_CASES = {
    "ks":     dict(shape=(64, 4, 80, 256, 32, 50), sched=("ks",) * 3, ups=None, rc=(False, True)),
    "T20":    dict(shape=(64, 20, 80, 256, 32, 50), sched=("ks",) * 3, ups=("loss", "log_px_z"), rc=(False,)),
    "rs":     dict(shape=(1024, 3, 80, 256, 32, 300), sched=("rs",) * 3, ups=("loss", "log_px_z", "neg_kld_z1"), rc=(False,)),
    "rows":   dict(shape=(1500, 3, 80, 128, 32, 300), sched=("rows",) * 3, ups=("loss", "log_px_z"), rc=(False,)),
    "cells":  dict(shape=(48, 5, 80, 64, 16, 40), sched=("cells",) * 3, ups=None, rc=(False,)),
    "big":    dict(shape=(256, 4, 80, 512, 32, 100), sched=("big",) * 3, ups=("loss", "log_px_z"), rc=(False,), env={"FHVAE_BIG_CELLS": "1"}),
    "f32heads": dict(shape=(48, 4, 6, 64, 4, 9), sched=("cells",) * 3, ups=("loss",), rc=(False,)),
}
# the rounding-model options of each schedule (oracle/lstm_lp_ref.py cites the kernel lines; as test_lstm_lp_oracle_gpu)
SCHED_OPTS = {"rs": dict(partial_dh_bf16=True), "rows": {}, "ks": {},
              "cells": dict(bias_from_rounded_dg=True),
              "big": dict(bias_from_rounded_dg=True, dgsum_from_rounded_dg=True)}


CLASSES = ("out", "lstm_w", "lstm_b", "head_w", "head_b", "table")


def _raised(**kw):
    """lstm_lp_compare.BF16 with the named constants replaced ("floor", or "<kind>_<measure>")."""
    c = copy.deepcopy(BF16)
    for k, v in kw.items():
        if k == "floor":
            c["floor"] = v
        else:
            kind, m = k.split("_")
            assert v > c[kind][m], k  # a constant only ever moves up, and only where the floor forced it
            c[kind][m] = v
    return c


# The floor: the bf16 oracle against itself with its biases and both eps moved by 1e-7, at the seven shapes of FLOOR_CASES
# (tests/test_step_oracle_cpu.py), five seeds each, every upstream of the case.  A whole step chains three nets and three heads,
# so a one-ulp flip of rb(.) in the decoder travels through the z1 and the z2 encoder too, and under a single-term upstream
# (log_px_z above all) nothing larger drowns it: the noise is 2x to 4x what one recurrence shows in lstm_lp_compare, and it is
# the same from seed to seed (worst mean on the LSTM weights: T = 20 1.2e-4 .. 1.6e-4, H = 512 0.9e-4 .. 1.1e-4, B = 64 T = 4
# 0.8e-4 .. 0.9e-4), so no choice of seed or table brings a family under a third of lstm_lp_compare.BF16.  The head biases (32
# to 160 elements) and the six outputs (B elements, one for log_qy) are too small for the mean and the signed mean to average
# over the flips.  Each constant below is 3x the worst floor measured for its class; every other one is lstm_lp_compare.BF16's.
#   class    measured max / mean / signed / worst bin - 8 x median bin    (BF16: 1e-2 / 2.5e-4 / 2e-5 / 1.5e-4)
#   out      7.2e-4 / 6.8e-5 / 2.0e-5 / -
#   lstm_w   3.7e-3 / 1.6e-4 / 2.3e-6 / 2.5e-4
#   lstm_b   2.7e-3 / 1.7e-4 / 1.6e-5 / 5.2e-4
#   head_w   3.3e-3 / 2.5e-4 / 8.8e-6 / 6.2e-6
#   head_b   3.3e-3 / 7.4e-4 / 1.9e-4 / -
#   table    3.7e-5 / 7.7e-7 / 1.1e-7 / 1.8e-7
STEP_BF16 = {"out": _raised(fwd_signed=6e-5),
             "lstm_w": _raised(grad_max=1.1e-2, grad_mean=4.8e-4, floor=7.5e-4),
             "lstm_b": _raised(grad_mean=5.1e-4, grad_signed=4.8e-5, floor=1.6e-3),
             "head_w": _raised(grad_mean=7.5e-4, grad_signed=2.7e-5),
             "head_b": _raised(grad_mean=2.3e-3, grad_signed=5.7e-4),
             "table": _raised()}
# f32 mode against the rounding-off oracle: lstm_lp_compare.F32 for every class
STEP_F32 = {c: F32 for c in CLASSES}


def class_of(name):
    if name in OUT:
        return "out"
    if name == "mu2_table":
        return "table"
    net = name.split(".")[0] in NETS
    bias = name.split(".")[-1].startswith("bias")
    return ("lstm_" if net else "head_") + ("b" if bias else "w")


def make_case(shape, seed):
    """Seeded CPU f32 inputs of one step: a FHVAERef state dict (torch.nn.LSTM's initialisation), x, idx with a repeated index
    (idx[1] = idx[0]), per-row num_segs, the table ~ N(0, 1), and both eps."""
    B, T, F, H, D, S = shape
    torch.manual_seed(seed)
    ref = R.FHVAERef(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, T, F, generator=g)
    idx = torch.randint(0, S, (B,), generator=g)
    idx[1] = idx[0]
    ns = torch.randint(3, 100, (B,), generator=g)
    table = torch.randn(S, D, generator=g)
    e2, e1 = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)
    return {"shape": shape, "ref": ref, "sd": {k: v.detach().clone() for k, v in ref.state_dict().items()}, "x": x, "idx": idx, "ns": ns,
            "table": table, "eps": (e2, e1)}


def upstreams(B, reference_compat, seed=0):
    """name -> upstream (oracle/fhvae_step_ref.step_bwd): the loss at alpha = 10, and seeded per-row weights on single terms of
    the 6-tuple; from neg_kld_z1 alone the only way into the z2 encoder is the z1 encoder's input gradient, from log_px_z alone
    the decoder's and (through z1_sample) the z1 encoder's; under lower_bound alone the table's gradient is the gather's, where
    a prior term kept under reference_compat shows (with log_qy beside it the discriminative gradient covers it).  Terms
    without a gradient under reference_compat are left out."""
    g = torch.Generator().manual_seed(1000 + seed)
    w = lambda: -(0.5 + torch.rand(B, generator=g, dtype=torch.float64)) / B
    ups = {"loss": ALPHA}
    wpx = w()
    if not reference_compat:
        ups["log_px_z"] = {"log_px_z": wpx}
    ups["neg_kld_z1"] = {"neg_kld_z1": w()}
    ups["neg_kld_z2"] = {"neg_kld_z2": w()}
    ups["lb+qy"] = {"lower_bound": w(), "log_qy": -3.0}
    ups["lower_bound"] = {"lower_bound": w()}
    return ups


def objective(out6, upstream):
    """The scalar whose gradient `upstream` describes, from a 6-tuple of torch tensors (any device, autograd)."""
    if not isinstance(upstream, dict):
        return -1 * torch.mean(out6[0] + float(upstream) * out6[1])
    total = 0
    for k, v in upstream.items():
        o = out6[OUT.index(k)]
        total = total + (o * v if k == "log_qy" else (o * torch.as_tensor(v).to(device=o.device, dtype=o.dtype)).sum())
    return total


def group_of(name):
    if name in OUT:
        return "outputs"
    if name == "mu2_table":
        return "table"
    head = name.split(".")[0]
    return head if head in NETS else "heads"


def _leaf(name):
    """The name lstm_lp_compare.bin_divisors sees: weight_ih_l0 ..., weight / bias of a head, the output's or the table's own."""
    return name.split(".")[-1]


def flatten(res):
    """{"out", "grads", "table"} -> name -> tensor or None (the table under "mu2_table")."""
    flat = {n: res["out"][n] for n in OUT if n in res["out"]}
    flat.update(res["grads"])
    flat["mu2_table"] = res["table"]
    return flat


def compare(got, want, consts, label="", quiet=False, table=None, scales=None):
    """got, want: {"out": name -> tensor, "grads": state-dict name -> tensor or None, "table": tensor or None}; consts: class
    (CLASSES) -> constants like lstm_lp_compare.BF16 (STEP_BF16, STEP_F32).  Every tensor of `want` is measured; where `want` has no gradient, `got` must have none (None or all zeros: a kernel that always writes its
    output, such as the lower bound's backward, hands autograd zeros).  scales: name -> the scale of that tensor in place of
    max |oracle| (the f32 cases: neg_kld_z1 of an untrained model is 0.5 sum_j 1 + lv - mu^2 - e^lv with every term near 1 and a
    sum near 0, so one f32 rounding per term, 2^-24 of the terms' magnitudes, is 1e-6 of the value; the oracle's a_out is that
    magnitude, as tests/head_elbo_compare.py scales the same outputs).  Returns the failures; `table` (a dict) receives, per
    tensor group, the worst max / mean / signed."""
    bad = []
    g, w = flatten(got), flatten(want)
    for name, wt in w.items():
        gt = g.get(name)
        if wt is None:
            if gt is not None and bool(gt.detach().double().abs().sum() > 0):
                bad.append("%s %s: a gradient where the oracle has none" % (label, name))
            continue
        if gt is None:
            bad.append("%s %s: no gradient" % (label, name))
            continue
        gt, wt = gt.detach().cpu().double(), wt.detach().cpu().double()
        if wt.dim() == 0:
            gt, wt = gt.reshape(1), wt.reshape(1)
        st = measure(_leaf(name), gt, wt)
        st["name"] = name
        if scales and name in scales:
            r = st["scale"] / scales[name]
            st.update({k: st[k] * r for k in ("max", "mean", "signed", "bin_max", "bin_med")}, scale=scales[name])
        f = failures(st, consts[class_of(name)], "fwd" if name in OUT else "grad")
        if not quiet:
            print("%s %s%s" % (label, fmt(st), ("  FAIL: " + "; ".join(f)) if f else ""))
        if table is not None:
            row = table.setdefault(group_of(name), {"max": 0.0, "mean": 0.0, "signed": 0.0})
            for k in row:
                row[k] = max(row[k], st[k])
        bad += ["%s %s: %s" % (label, name, x) for x in f]
    return bad


def print_table(label, table):
    for grp, row in table.items():
        print("STEPTABLE | %s | %s | %.2e %.2e %.2e" % (label, grp, row["max"], row["mean"], row["signed"]))
