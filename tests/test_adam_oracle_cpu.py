"""The float64 oracle of the fused Adam step (oracle/adam_ref.py) and the comparator of the GPU checks (tests/adam_compare.py), on
the CPU: the oracle is torch.optim.Adam in float64; a float32 emulation of the kernel's expressions in the kernel's order
(csrc/loss.hip adam_one :384-392 and the two bias corrections of :407) passes compare() on every input family, step count, beta
pair and gradient scale tests/test_adam_oracle_gpu.py uses, no element left out; and every deliberately wrong variant of that
emulation is rejected on at least one of those cases.

Measured here (the emulation, all 68 cases): worst ratio p 0.998 (the store's rounding: u |p| is half an ulp where the mantissa is
1.0), m 0.51, v 0.48, dp 0.18 of the bounds; the wrong variants land 3.8e3 times and more above them.
"""
import numpy as np
import pytest
import torch

import adam_compare as AC
from oracle.adam_ref import adam_ref_run, adam_ref_step, f32

BETAS = [(0.95, 0.999), (0.9, 0.99), (0.0, 0.999)]
STEPS = [1, 2, 3, 10, 1000, 100000]
SCALES = [1.0, 1.0 / 8, 1.0 / 3]
HYPER = [(3e-4, 1e-6), (1e-3, 1e-8)]  # (lr, eps): distinct values, so that a swapped argument shows
BIG = AC.GRID_CAP_ELEMS + 1029

F = np.float32


def emulate(c: dict, t, lr, b1, b2, eps, s=1.0, fault=None) -> dict:
    """The kernel's f32 arithmetic in numpy (one rounding per operation, no contraction).  c: f32 p, g, m, v.  fault: a wrong
    variant, for the comparator's own tests."""
    p, g, m, v = (c[k].numpy().copy() for k in ("p", "g", "m", "v"))
    lr, b1, b2, eps, s, one = F(lr), F(b1), F(b2), F(eps), F(s), F(1)
    with np.errstate(all="ignore"):
        bc1 = one - np.power(b1, F(t))
        bc2 = one - np.power(b2, F(t - 1 if fault == "bc2_one_step_late" else t))
        lr_bc1 = lr if fault == "no_bc1" else lr / bc1
        rs_bc2 = one / np.sqrt(bc2)
        gi = g * s
        gv = g if fault == "scale_m_only" else gi           # both factors of v's gi^2 unscaled
        gv2 = g if fault == "v_from_g" else gv               # v's second factor is g in place of g s
        m1 = b1 * m + (one - b1) * gi
        v1 = b2 * v + (one - b2) * gv * gv2
        if fault == "eps_in_sqrt":
            denom = np.sqrt(v1 + eps) * rs_bc2
        elif fault == "eps_before_bc2":
            denom = (np.sqrt(v1) + eps) * rs_bc2
        else:
            denom = np.sqrt(v1) * rs_bc2 + eps
        p1 = p - lr_bc1 * (m1 / denom)
    n = p.shape[0]
    keep = slice(0, 0)
    if fault == "tail_untouched":
        keep = slice(n - n % 4, n)
    elif fault == "past_grid_untouched":
        keep = slice(AC.GRID_CAP_ELEMS, n)
    for new, old in ((p1, p), (m1, m), (v1, v)):
        new[keep] = old[keep]
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    return {"p": torch.from_numpy(p1), "m": torch.from_numpy(m1), "v": torch.from_numpy(v1)}


def cases():
    """(label, n, t, (b1, b2), s, (lr, eps), kind, warm, v_abs): the families, step counts, beta pairs and scales of the GPU file."""
    out = []
    for bi, betas in enumerate(BETAS):
        for ti, t in enumerate(STEPS):
            for si, s in enumerate(SCALES):
                out.append(("grid", 1027, t, betas, s, HYPER[(bi + ti + si) % 2], "mixed", 3, None))
    for n in (1, 2, 3, 4, 5, 7, 1023, 1024, 1027, 4 * 256 * 65 + 2):
        out.append(("size", n, 3, BETAS[0], 1.0, HYPER[0], "mixed", 3, None))
    out.append(("zero state", 1027, 1, BETAS[0], 1.0, HYPER[0], "mixed", 0, None))
    out.append(("tiny g", 1027, 3, BETAS[0], 1.0, HYPER[1], "tiny", 3, AC.V_TINY))
    out.append(("zero g", 1027, 1, BETAS[0], 1.0, HYPER[1], "zero", 0, None))
    out.append(("grid cap", BIG, 4, BETAS[0], 1.0 / 8, HYPER[0], "mixed", 1, None))
    return out


CASES = cases()
_made = {}


def _case(c):
    label, n, t, (b1, b2), s, (lr, eps), kind, warm, v_abs = c
    key = (n, b1, b2, s, kind, warm)
    if key not in _made:
        if n == BIG:
            _made.pop(next((k for k in _made if k[0] == BIG), None), None)  # one large case at a time
        _made[key] = AC.make_case(n, 1000 + n % 997 + len(kind), b1, b2, s, kind, warm)
    return _made[key]


def _run(c, fault=None):
    label, n, t, (b1, b2), s, (lr, eps), kind, warm, v_abs = c
    before = _case(c)
    return AC.compare(before, emulate(before, t, lr, b1, b2, eps, s, fault), t, lr, b1, b2, eps, s, v_abs)


def test_oracle_is_torch_adam_in_float64():
    """20 steps of torch.optim.Adam on float64 parameters with the rounded hyper-parameters over g s: p, m, v to 1e-12 relative."""
    n, lr, (b1, b2), eps, s = 517, 3e-4, BETAS[0], 1e-6, 1.0 / 3
    gen = torch.Generator().manual_seed(5)
    p0 = AC.make_case(n, 5, b1, b2)["p"]
    grads = [AC.make_grad(n, gen, s, phase=k) for k in range(20)]
    ref = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=f32(lr), betas=(f32(b1), f32(b2)), eps=f32(eps))
    for g in grads:
        ref.grad = g.double() * f32(s)
        opt.step()
    p, m, v = adam_ref_run(p0, grads, lr, b1, b2, eps, s)
    st = opt.state[ref]
    for name, got, want in (("p", p, ref.detach()), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
        rel = ((got - want).abs() / want.abs().clamp_min(1e-300)).max().item()
        assert rel <= 1e-12, (name, rel)
    # ... and one step returns the update it applied
    p1, _, _, d = adam_ref_step(p0, grads[0], torch.zeros(n), torch.zeros(n), 1, lr, b1, b2, eps, s)
    assert torch.equal(p0.double() - d, p1)


def test_emulated_kernel_passes_every_case():
    """The reference arithmetic alone stays inside the bounds: every family, size, step count, beta pair and scale, no exclusions."""
    worst = dict.fromkeys(AC.KEYS, 0.0)
    for c in CASES:
        r = _run(c)
        assert not AC.bad(r), (c[:7], AC.fmt(r), r["at"])
        for k in AC.KEYS:
            worst[k] = max(worst[k], r[k])
    print("emulation, worst ratio over %d cases: %s" % (len(CASES), "  ".join("%s %.3f" % kv for kv in worst.items())))
    # zero gradient from a zero state: nothing moves
    z = next(c for c in CASES if c[0] == "zero g")
    out = emulate(_case(z), 1, 1e-3, 0.95, 0.999, 1e-8)
    assert torch.equal(out["p"], _case(z)["p"]) and not out["m"].any() and not out["v"].any()


# the listed wrong variants and where each must show (label, t, s filters over CASES; None: any)
MUTANTS = {
    "eps_in_sqrt": ("grid", None, None),
    "eps_before_bc2": ("grid", 10, None),
    "bc2_one_step_late": ("grid", 10, None),
    "no_bc1": ("grid", 10, None),
    "scale_m_only": ("grid", None, 1.0 / 3),
    "v_from_g": ("grid", None, 1.0 / 8),
    "tail_untouched": ("size", None, None),
    "past_grid_untouched": ("grid cap", None, None),
}


@pytest.mark.parametrize("fault", sorted(MUTANTS))
def test_comparator_rejects(fault):
    label, t, s = MUTANTS[fault]
    sel = [c for c in CASES if c[0] == label and (t is None or c[2] == t) and (s is None or c[4] == s)]
    if fault == "tail_untouched":
        sel = [c for c in sel if c[1] % 4]
    if fault == "no_bc1":
        sel = [c for c in sel if c[3][0] > 0]  # (b1 = 0 has no first correction)
    assert sel
    ratios = [_run(c, fault) for c in sel]
    assert all(AC.bad(r) for r in ratios), [(c[:6], AC.fmt(r)) for c, r in zip(sel, ratios) if not AC.bad(r)]
    print("%s: smallest worst ratio %.3g over %d cases" % (fault, min(max(r[k] for k in AC.KEYS) for r in ratios), len(sel)))


def test_first_bias_correction_is_one_from_t_1000_on():
    """The issue lists `the first bias correction missing at t = 1000`.  With the beta pairs in use b1^1000 <= 0.95^1000 = 5e-23:
    1 - b1^t is 1 to 1e-22 in float64 and exactly 1 in f32, so the correction is not there to be missed and no comparator can see
    the variant at that step (pinned here); test_comparator_rejects takes it at t = 10, the largest listed step where it exists."""
    for c in CASES:
        if c[0] == "grid" and c[2] >= 1000:
            assert not AC.bad(_run(c, "no_bc1"))
