"""Float64 Adam with the arithmetic of the fused HIP step (fhvae_adam_step: csrc/loss.hip adam_one :653-661, adam_kernel :670-727).

One step from a given state, t the step count the launch uses (step[0], or step[0] + 1 with FHVAE_ADAM_ADVANCE, loss.hip:673):
    gi = g s                                   (:655, s = grad_scale: the 1/W of data-parallel training)
    m  = b1 m + (1 - b1) gi                    (:656)
    v  = b2 v + (1 - b2) gi^2                  (:657)
    denom = sqrt(v) / sqrt(1 - b2^t) + eps     (:658 with rs_bc2 of :676: eps outside the root and behind the bias correction)
    p  = p - lr / (1 - b1^t) (m / denom)       (:659 with lr_bc1 of :676)
which is torch.optim.Adam (no weight decay, no amsgrad) over the gradient g s.

The hyper-parameters lr, b1, b2, eps and s enter as the f32 values the C ABI receives (`f32()`): the kernel is self-consistent in
its rounded betas (the same b2 multiplies v and sits in 1 - b2^t), so exact Adam with the rounded values is the target.  Everything
else is float64: the products, 1 - b^t, both roots, the quotient.  p, g, m, v are taken as they are (the kernel's f32 values are
exact in float64), so a step from the device's own state has no history in it.

`adam_ref_run` repeats the step over a list of gradients (the trajectory torch.optim.Adam follows in float64).
"""
from typing import Sequence

import torch


def f32(x: float) -> float:
    """x as the `float` argument of the C ABI holds it."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def adam_ref_terms(g, m, v, t, lr, b1, b2, eps, grad_scale=1.0) -> dict:
    """The step's float64 intermediates (tests/adam_compare.py builds its bounds from them): gi, m, v, bc1 = 1 - b1^t,
    bc2 = 1 - b2^t, root = sqrt(v) / sqrt(bc2), denom = root + eps, delta = lr / bc1 * m / denom, and the rounded hyper-parameters."""
    lr, b1, b2, eps, s = (f32(x) for x in (lr, b1, b2, eps, grad_scale))
    t = int(t)
    gi = g.detach().double() * s
    m = b1 * m.detach().double() + (1.0 - b1) * gi
    v = b2 * v.detach().double() + (1.0 - b2) * gi * gi
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    root = v.sqrt() / bc2 ** 0.5
    denom = root + eps
    delta = (lr / bc1) * (m / denom)
    return {"gi": gi, "m": m, "v": v, "bc1": bc1, "bc2": bc2, "root": root, "denom": denom, "delta": delta,
            "lr": lr, "b1": b1, "b2": b2, "eps": eps, "s": s}


def adam_ref_step(p, g, m, v, t, lr, b1, b2, eps, grad_scale=1.0):
    """One step from (p, g, m, v) at step count t.  Returns float64 p, m, v and the update delta = p_before - p_after."""
    T = adam_ref_terms(g, m, v, t, lr, b1, b2, eps, grad_scale)
    return p.detach().double() - T["delta"], T["m"], T["v"], T["delta"]


def adam_ref_run(p, grads: Sequence[torch.Tensor], lr, b1, b2, eps, grad_scale=1.0, t0=0, m=None, v=None):
    """Steps t0 + 1 ... t0 + len(grads) from (p, m, v) (the moments default to 0).  Returns float64 p, m, v."""
    p = p.detach().double()
    m = torch.zeros_like(p) if m is None else m.detach().double()
    v = torch.zeros_like(p) if v is None else v.detach().double()
    for k, g in enumerate(grads):
        p, m, v, _ = adam_ref_step(p, g, m, v, t0 + k + 1, lr, b1, b2, eps, grad_scale)
    return p, m, v
