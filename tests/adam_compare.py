"""One comparator for the fused Adam step (fhvae_adam_step, csrc/loss.hip:384-458) against its float64 oracle (oracle/adam_ref.py):
tests/test_adam_oracle_gpu.py checks the kernel with it, tests/test_adam_oracle_cpu.py checks that a float32 emulation of the
kernel's arithmetic passes it everywhere and that it rejects the errors a kernel could hide.

The comparison is ONE step from the device's own state: p, g, m, v are copied to the CPU before the launch, the oracle steps from
exactly those f32 values, and the results are compared after the launch.  Nothing accumulates, so every bound is a rounding bound
of the kernel's own expression, first order in u = 2^-24 (one f32 rounding to nearest).  t is the step the launch uses; b1, b2,
lr, eps, s are the f32 hyper-parameters, the same in the kernel and in the oracle; subscript o is the oracle's value, k the
kernel's.

m = b1 m0 + (1 - b1) gi, gi = fl(g s)                                                   |m_k - m_o| <= 4u (|b1 m0| + |(1 - b1) g s|)
    1 - b1 is exact in f32 (b1 >= 0.5 or b1 = 0).  The first term carries its product's and the sum's rounding (2u), the second
    gi's, its product's and the sum's (3u); an FMA contraction removes a product's rounding.  4u covers both.
v = b2 v0 + ((1 - b2) gi) gi                                                             |v_k - v_o| <= 6u v_o
    every term is non-negative.  First term 2u, second 2u (gi twice) + 2u (two products) + u (the sum) = 5u.  The input ranges
    keep (1 - b2) gi^2 a normal f32.  Where gi^2 underflows (the |g| <= 1e-20 case) no relative bound holds; the caller passes
    v_abs = 2^-126 and the bound is absolute.
delta = lr_bc1 (m / denom), lr_bc1 = lr / (1 - b1^t), denom = sqrt(v) rs_bc2 + eps, rs_bc2 = 1 / sqrt(1 - b2^t)
    relative to delta_o:   (bound of m) / |m_o|                the numerator
                         + (1/2) 6u                            v's error through the root (weighted by root / denom <= 1)
                         + 6u                                  the roundings behind m and v, see below
                         + 4u / (1 - b1^t)                     1 - powf(b1, t): b^t < 1 has ulp <= u, powf allowed 3 ulp, the
                                                               subtraction u
                         + (1/2) 4u / (1 - b2^t)               the same under the root
    The last two terms are the f32 bias corrections, the one place where the kernel is legitimately far from float64: 1.2e-4 at
    t = 1 with b2 = 0.999, 4e-7 by t = 1000.  The bound is evaluated as an absolute one,
        bd = bm (lr / bc1) / denom_o + |delta_o| (3u + 6u + 4u / bc1 + 2u / bc2),
    so that m_o = 0 (g = 0 from a zero state) needs no special case: there bd = 0 and the kernel's update must be 0.
    Counting the roundings behind m and v one by one gives 8: lr / bc1, sqrtf(bc2), 1 / that, sqrtf(v), its product with rs_bc2,
    the sum with eps, m / denom, the product with lr_bc1 (hipcc's sqrtf and division are correctly rounded).  The issue that set
    these constants allows 6u; the constant is kept as set.  The two bias-correction terms allow powf 3 ulp where the device
    library documents 1, which leaves at least 2u + u of real slack over the two the count exceeds 6u by, and at t = 1 powf(b, 1)
    is b.  tests/test_adam_oracle_cpu.py runs the emulation (the same eight roundings) through every case; the worst ratio it
    and the kernel reach are recorded there and in the GPU test's docstring.
p = fl(p0 - delta)                                                                       |p_k - p_o| <= u |p_o| + bd
    the store's rounding and the update's error.

The kernel does not return delta; it is observed as p0 - p_k (exact in float64), which carries the store's rounding u |p_o|.  The
delta ratio is therefore what is left of the error after that rounding is granted in full, over the update's own bound,
max(0, |p0 - p_k - delta_o| - u |p_o|) / bd: where p0 = 0 (one element in eight of the mixed family) the store is exact
(0 - x = -x) and the ratio is the update's alone, at about 1e-7 relative.  It passes exactly when p's does; it reads differently.

A ratio is error / bound; with a bound of 0 it is 0 for an exact result and inf otherwise.  A non-finite result is inf.

`trajectory` is the many-step form for hip_optim.FusedAdam: the oracle's run over a list of gradients and, per element, the sum
over the steps of that step's p bound (u |p_o| + bd).  Each step's bias-correction allowance (2080u, 1041u, 694u ... of |delta| for
t = 1, 2, 3 ... with the reference's betas) is far above the drift of the kernel's f32 moments from the oracle's, a few u per step.
"""
import torch

from oracle.adam_ref import adam_ref_terms, f32

U = 2.0 ** -24
V_TINY = 2.0 ** -126
KEYS = ("p", "m", "v", "dp")
GRID_CAP_ELEMS = 8192 * 256 * 4  # one pass of the capped grid: 8192 workgroups x 256 lanes x 4 elements (loss.hip:652-653)


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _logu(n, lo, hi, gen):
    """n magnitudes log-uniform in [10^lo, 10^hi] with random signs, float64."""
    mag = 10.0 ** (lo + (hi - lo) * torch.rand(n, generator=gen, dtype=torch.float64))
    return mag * (torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1)


def make_grad(n, gen, s=1.0, kind="mixed", phase=0):
    """An f32 gradient whose product with grad_scale is log-uniform in [1e-12, 1e12] (both sides of sqrt(v_hat) = eps; (1 - b2) gi^2
    stays a normal f32 below overflow), one element in eight exactly 0.  kind "tiny": |g| in [1e-30, 1e-20], gi^2 underflows."""
    lo, hi = (-12.0, 12.0) if kind == "mixed" else (-30.0, -20.0)
    g = (_logu(n, lo, hi, gen) / f32(s)).float()
    g[(torch.arange(n) + phase) % 8 == 5] = 0.0
    return g


def make_case(n, seed, b1, b2, s=1.0, kind="mixed", warm=3) -> dict:
    """f32 p, g, m, v on the CPU.  |p| log-uniform in [1e-6, 10], one element in eight exactly 0 (there the new p is -delta rounded);
    g as make_grad; m, v the oracle's moments after `warm` steps over fresh gradients of the same family, rounded to f32 (warm = 0: zeros).
    kind "zero": g = 0."""
    gen = torch.Generator().manual_seed(seed)
    p = _logu(n, -6.0, 1.0, gen).float()
    p[torch.arange(n) % 8 == 3] = 0.0
    gk = "mixed" if kind == "zero" else kind
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for k in range(warm):
        T = adam_ref_terms(make_grad(n, gen, s, gk, phase=k + 1), m, v, k + 1, 1e-3, b1, b2, 1e-8, s)
        m, v = T["m"], T["v"]
    g = torch.zeros(n) if kind == "zero" else make_grad(n, gen, s, gk)
    return {"p": p, "g": g, "m": m.float(), "v": v.float()}


# ---------------------------------------------------------------------------------------------
# bounds and ratios
# ---------------------------------------------------------------------------------------------
def bounds(before: dict, t, lr, b1, b2, eps, grad_scale=1.0, v_abs=None) -> dict:
    """The oracle's step from `before` (f32 p, g, m, v) and the bound of each output (module docstring): want p, m, v, dp and
    bound p, m, v, dp, float64."""
    T = adam_ref_terms(before["g"], before["m"], before["v"], t, lr, b1, b2, eps, grad_scale)
    m0 = before["m"].double()
    bm = 4 * U * ((T["b1"] * m0).abs() + ((1.0 - T["b1"]) * T["gi"]).abs())
    bv = torch.full_like(bm, float(v_abs)) if v_abs is not None else 6 * U * T["v"]
    rel = 3 * U + 6 * U + 4 * U / T["bc1"] + 2 * U / T["bc2"]
    bd = bm * (T["lr"] / T["bc1"]) / T["denom"] + T["delta"].abs() * rel
    p_o = before["p"].double() - T["delta"]
    return {"want": {"p": p_o, "m": T["m"], "v": T["v"], "dp": T["delta"]},
            "bound": {"p": U * p_o.abs() + bd, "m": bm, "v": bv, "dp": bd}}


def ratio(err, bound):
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return torch.nan_to_num(r, nan=float("inf"), posinf=float("inf"))


def compare(before: dict, after: dict, t, lr, b1, b2, eps, grad_scale=1.0, v_abs=None) -> dict:
    """before: f32 p, g, m, v as the launch found them; after: p, m, v as it left them (any device).  Returns the worst ratio
    error / bound of p, m, v and dp (the update, observed as p_before - p_after), "at" (the element of each worst ratio) and
    "finite".  No element is left out."""
    B = bounds(before, t, lr, b1, b2, eps, grad_scale, v_abs)
    got = {k: after[k].detach().cpu().double().reshape(-1) for k in ("p", "m", "v")}
    out = {"finite": all(bool(torch.isfinite(x).all()) for x in got.values()), "at": {}, "n": got["p"].numel(), "t": int(t)}
    err = {k: (got[k] - B["want"][k]).abs() for k in got}
    # the update through the stored p: what the store's rounding does not account for
    err["dp"] = ((before["p"].double() - got["p"]) - B["want"]["dp"]).abs() - U * B["want"]["p"].abs()
    err["dp"] = torch.where(torch.isnan(err["dp"]), err["dp"], err["dp"].clamp_min(0.0))
    for k in KEYS:
        r = ratio(err[k], B["bound"][k])
        i = int(r.argmax())
        out[k], out["at"][k] = float(r[i]), i
    return out


def fmt(r: dict) -> str:
    return "n %d t %d   p %.3f  m %.3f  v %.3f  dp %.3f%s" % (r["n"], r["t"], r["p"], r["m"], r["v"], r["dp"], "" if r["finite"] else "  NOT FINITE")


def bad(r: dict) -> list:
    """The names of the outputs over their bound (empty: the step passes)."""
    return [k for k in KEYS if not r[k] <= 1.0] + ([] if r["finite"] else ["finite"])


def check(r: dict, label: str):
    """Print the case's ratios, then assert every one is within its bound."""
    print("adam %-34s %s" % (label, fmt(r)))
    assert not bad(r), "%s: over the bound: %s (worst elements %s)   %s" % (label, bad(r), r["at"], fmt(r))
    return r


def trajectory(p0, grads, lr, b1, b2, eps, grad_scale=1.0):
    """The oracle over steps 1 .. len(grads) from p0 with zero moments.  Returns float64 p, m, v and, per element, the sum of the
    steps' p bounds."""
    p = p0.detach().double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    total = torch.zeros_like(p)
    for k, g in enumerate(grads):
        B = bounds({"p": p, "g": g, "m": m, "v": v}, k + 1, lr, b1, b2, eps, grad_scale)
        total += B["bound"]["p"]
        p, m, v = B["want"]["p"], B["want"]["m"], B["want"]["v"]
    return p, m, v, total
