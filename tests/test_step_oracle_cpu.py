"""The composed float64 oracle of one FHVAE training step (oracle/fhvae_step_ref.py) and the comparator of the GPU check
(tests/step_compare.py), on the CPU:

  composition  with rounding off, the chain of per-kernel oracles IS FHVAERef(...).double() under autograd, for the loss and for
               every single-term upstream, at both reference_compat values: outputs and gradients within 1e-12 of scale; the
               gradients the discriminative gradient feeds (z2 encoder, z2 head, table, under an upstream with log_qy) within
               2^-22, because disc_ref_bwd forms its upstream factor as the kernels' f32 product (two f32 roundings, margin 2);
               a gradient autograd reports as None is None in the oracle.
  floor        the bf16 oracle against itself with its biases and both eps moved by 1e-7 (what another f32 accumulation order
               does to a kernel's sums), per upstream, at the smallest case of each schedule family and at T = 20: the noise
               stays under one third of step_compare.STEP_BF16 in every measure.  Those are lstm_lp_compare.BF16 except where
               this floor forced a constant up, to 3x what was measured over five seeds (the comment beside STEP_BF16).
  rejection    every _fault of the oracle fails the comparator under at least one upstream of the set, named in FAULTS.
  sanity       the bf16 oracle's outputs track the float64 ones within the 1e-2 of the existing bf16 tests.

Measured floors at the seed the test runs (worst tensor over the upstreams of the case; max / mean / signed of scale; the
worst tensor is a head bias under log_px_z in every bf16-head case):
  ks       (64, 4, 80, 256, 32, 50)      2.8e-3 / 4.5e-4 / 3.9e-5
  rs       (1024, 3, 80, 256, 32, 300)   1.2e-3 / 2.3e-4 / 3.4e-5
  rows     (1500, 3, 80, 128, 32, 300)   9.3e-4 / 1.8e-4 / 4.2e-5
  cells    (48, 5, 80, 64, 16, 40)       2.0e-3 / 2.2e-4 / 5.1e-5
  big      (256, 4, 80, 512, 32, 100)    2.1e-3 / 6.3e-4 / 5.4e-5
  f32heads (48, 4, 6, 64, 4, 9)          5.1e-4 / 1.4e-5 / 4.7e-6
  T20      (64, 20, 80, 256, 32, 50)     2.7e-3 / 5.1e-4 / 1.8e-4
Per tensor class over five seeds: the table beside step_compare.STEP_BF16.  Composition, measured: 1.4e-15 of scale, and 1.2e-7
on the gradients the discriminative gradient feeds.  Under the training loss alone the z1 encoder's dropped share of d z2_sample
passes (test_loss_alone_misses_a_dropped_share).
"""
import copy

import pytest
import torch

import step_compare as SC
from oracle.fhvae_step_ref import NETS, OUT, disc_mode_for, step_bwd, step_fwd


def _oracle_fwd(case, rc, rounding, sched=("ks",) * 3, fault=None, sd=None, eps=None):
    B, T, F, H, D, S = case["shape"]
    return step_fwd(sd or case["sd"], case["x"], case["idx"], case["ns"], case["table"], eps or case["eps"], rc, rounding=rounding,
                    net_opts={n: SC.SCHED_OPTS[s] for n, s in zip(NETS, sched)}, disc_mode=disc_mode_for(B, S, D, True), _fault=fault)


def _result(ctx, up):
    r = step_bwd(ctx, up)
    r["out"] = ctx["out"]
    return r


# ------------------------------------------------------------------------------------------------------------------------------
# composition
# ------------------------------------------------------------------------------------------------------------------------------
def _autograd(case, rc, up):
    ref = copy.deepcopy(case["ref"]).double()
    table = case["table"].double().requires_grad_(True)
    S = table.shape[0]
    out = ref(case["x"].double(), case["idx"], S, case["ns"], mu2_table=table, eps_z2=case["eps"][0].double(),
              eps_z1=case["eps"][1].double(), reference_compat=rc)
    names = [n for n, _ in ref.named_parameters()]
    gs = torch.autograd.grad(SC.objective(out, up), [p for _, p in ref.named_parameters()] + [table], allow_unused=True)
    return {"out": {n: o.detach() for n, o in zip(OUT, out)}, "grads": dict(zip(names, gs[:-1])), "table": gs[-1]}


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("shape", [(5, 4, 6, 8, 4, 9), (7, 3, 16, 16, 8, 11)])
def test_unrounded_composition_is_float64_autograd(shape, rc):
    case = SC.make_case(shape, sum(shape))
    ctx = _oracle_fwd(case, rc, rounding=False)
    worst = {"exact": 0.0, "disc": 0.0}
    for uname, up in SC.upstreams(shape[0], rc).items():
        want, got = _autograd(case, rc, up), _result(ctx, up)
        with_qy = not isinstance(up, dict) or "log_qy" in up
        g, w = SC.flatten(got), SC.flatten(want)
        assert set(g) == set(w)
        for name, wt in w.items():
            if wt is None:
                assert g[name] is None, (uname, name)
                continue
            assert g[name] is not None, (uname, name)
            fed = with_qy and (name == "mu2_table" or name.split(".")[0] in ("z2_pre_encoder", "z2_gauss_layer"))
            err = (g[name] - wt).abs().max().item() / max(wt.abs().max().item(), 1e-300)
            worst["disc" if fed else "exact"] = max(worst["disc" if fed else "exact"], err)
            assert err <= (2.0 ** -22 if fed else 1e-12), (uname, name, err)
    print("composition %s rc=%s: worst %.2e (exact) %.2e (fed by the discriminative gradient)" % (shape, rc, worst["exact"], worst["disc"]))


# ------------------------------------------------------------------------------------------------------------------------------
# floor
# ------------------------------------------------------------------------------------------------------------------------------
THIRD = {cl: {k: ({m: v / 3 for m, v in c.items()} if isinstance(c, dict) else c / 3) for k, c in cs.items()}
         for cl, cs in SC.STEP_BF16.items()}
FLOOR_CASES = ["ks", "rs", "rows", "cells", "big", "f32heads", "T20"]


def _moved(case, seed):
    """The state dict with every bias, and both eps, moved by 1e-7 (float64: rb() of the oracle takes them through f32)."""
    g = torch.Generator().manual_seed(seed)
    sd = {k: (v.double() + torch.randn(v.shape, generator=g, dtype=torch.float64) * 1e-7 if v.dim() == 1 else v) for k, v in case["sd"].items()}
    eps = tuple(e.double() * (1 + torch.randn(e.shape, generator=g, dtype=torch.float64) * 1e-7) for e in case["eps"])
    return sd, eps


@pytest.mark.parametrize("cname", FLOOR_CASES)
def test_floor(cname):
    spec = SC.GPU_CASES[cname]
    case = SC.make_case(spec["shape"], 7)
    a = _oracle_fwd(case, False, True, spec["sched"])
    sd, eps = _moved(case, 3)
    b = _oracle_fwd(case, False, True, spec["sched"], sd=sd, eps=eps)
    bad, worst = [], {"max": 0.0, "mean": 0.0, "signed": 0.0, "bin": 0.0}
    ups = SC.upstreams(spec["shape"][0], False)
    for uname in spec["ups"] or ups:
        table = {}
        bad += SC.compare(_result(b, ups[uname]), _result(a, ups[uname]), THIRD, "floor %s %s" % (cname, uname), table=table)
        for row in table.values():
            for k in ("max", "mean", "signed"):
                worst[k] = max(worst[k], row[k])
    print("FLOOR | %s | %s | %.1e / %.1e / %.1e" % (cname, spec["shape"], worst["max"], worst["mean"], worst["signed"]))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------------
# rejection
# ------------------------------------------------------------------------------------------------------------------------------
# fault -> (reference_compat, an upstream under which the comparator reports it)
FAULTS = {"drop_dec_dz2": (False, "log_px_z"), "drop_z1_dz2": (False, "neg_kld_z1"), "drop_disc_dq": (False, "loss"),
          "drop_disc_dt": (False, "loss"), "drop_gather_dt": (False, "neg_kld_z2"), "z1_on_mu": (False, "loss"),
          "dec_swapped": (False, "loss"), "head_prev_step": (False, "loss"), "prior_kept": (True, "lower_bound"), "ce_sign": (False, "loss")}
_SHAPE = SC.GPU_CASES["ks"]["shape"]


@pytest.fixture(scope="module")
def clean():
    case = SC.make_case(_SHAPE, 7)
    return case, {rc: _oracle_fwd(case, rc, True) for rc in (False, True)}


def test_fault_list_covers_the_oracle():
    import oracle.fhvae_step_ref as M

    listed = {ln.split('"')[1] for ln in M.__doc__.splitlines() if ln.strip().startswith('{"')}
    assert listed == set(FAULTS)


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_comparator_rejects(clean, fault):
    case, ctx = clean
    rc, named = FAULTS[fault]
    wrong = _oracle_fwd(case, rc, True, fault={fault: True})
    failed = {}
    for uname, up in SC.upstreams(_SHAPE[0], rc).items():
        bad = SC.compare(_result(wrong, up), _result(ctx[rc], up), SC.STEP_BF16, "%s %s" % (fault, uname), quiet=True)
        if bad:
            failed[uname] = bad
    print("REJECT | %s | fails under: %s" % (fault, ", ".join(failed) or "nothing"))
    assert named in failed, "%s passed the comparator under %s (it fails under: %s)" % (fault, named, sorted(failed))


def test_loss_alone_misses_a_dropped_share(clean):
    """Why the upstream set has single terms: under the training loss the discriminative gradient dominates the z2 encoder, and
    d z2_sample without the z1 encoder's share passes."""
    case, ctx = clean
    wrong = _oracle_fwd(case, False, True, fault={"drop_z1_dz2": True})
    assert SC.compare(_result(wrong, SC.ALPHA), _result(ctx[False], SC.ALPHA), SC.STEP_BF16, "drop_z1_dz2", quiet=True) == []


# ------------------------------------------------------------------------------------------------------------------------------
# sanity
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [False, True])
def test_bf16_oracle_tracks_float64(clean, rc):
    case, ctx = clean
    exact = _oracle_fwd(case, rc, False)
    for n in OUT:
        w, g = exact["out"][n], ctx[rc]["out"][n]
        assert (g - w).abs().max().item() <= 1e-2 * w.abs().max().item(), n
