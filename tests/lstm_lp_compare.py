"""One comparator for the LSTM recurrences against the rounding-faithful float64 oracle (oracle/lstm_lp_ref.py), with one set of
constants per mode (bf16, f32) shared by every case and schedule: tests/test_lstm_lp_oracle_gpu.py checks the kernels with it,
tests/test_lstm_lp_oracle_cpu.py checks that it rejects bf16-level and localized errors.

Per tensor, scale = max |oracle|, error = got - oracle:
  max      max |error| / scale
  mean     mean |error| / scale
  signed   |mean error| / scale
  local    the mean |error| per bin (hs_top: (t, 32-row block, 64-unit block); hn, d_xc: (32-row block, 64-column block); weights:
           (gate, 64-unit block) x 64-column block; biases: (gate, 64-unit block)); the worst bin's mean may not exceed
           LOCAL_RATIO x the median bin's mean + floor x scale.  An error confined to one member, one step or one tail of rows
           stands out here long before it moves the tensor-wide numbers.
"""
import torch

LOCAL_RATIO = 8.0

# kind "fwd": hs_top, hn, the bf16 states; kind "grad": parameter gradients and d_xc.
# bf16: the oracle reproduces every rounding point, but not the f32 accumulation order of the kernels; a difference of one f32 ulp
# flips an occasional rb(h), rb(gate) or rb(dg) by one bf16 ulp, and the recurrence carries the flip on.  That noise is the floor of
# this comparison: the oracle against itself with its biases and g_out perturbed at 1e-7 (test_lstm_lp_oracle_cpu) differs by
# mean 2e-5 .. 8e-5 of scale on the gradients at T = 20, maxima of 1e-3, worst bins 10-35x the median bin on the second layer's
# biases, which is what the kernels show; with saturated gates at T = 40 the same self-comparison gives gradient means of 1.8e-4
# (the kernels: up to 1.55e-4).  The constants sit above that floor (the forward maximum: one bf16 ulp of hs_lp, 2^-7 of a
# value just below a power of two); the mean bound is 10x tighter than the 2.5e-3 of the f32 torch.nn.LSTM comparisons.
BF16 = {"fwd": {"max": 1e-2, "mean": 2.5e-4, "signed": 2e-5},
        "grad": {"max": 1e-2, "mean": 2.5e-4, "signed": 2e-5},
        "floor": 1.5e-4}
# f32 mode (exact-f32 products, no rounding points): measured max 1.5e-6, mean 2.5e-7, signed 4e-8 of scale
F32 = {"fwd": {"max": 2e-5, "mean": 2e-6, "signed": 5e-7},
       "grad": {"max": 5e-5, "mean": 2e-6, "signed": 5e-7},
       "floor": 2e-6}


def make_inputs(B, T, I, Ic, H, L, seed, w_scale=1.0, x_scale=1.0, wh_scale=1.0):
    """Seeded CPU f32 inputs of one lstm_seq run: x (T,B,I) or None, xc (B,Ic) or None, the flat per-layer parameters
    (torch.nn.LSTM's initialisation, U(-1/sqrt(H), 1/sqrt(H)); W_ih and the biases times w_scale, W_hh times wh_scale),
    g_out (T,B,H), g_hn (B,L*H)."""
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / H ** 0.5
    params = []
    for l in range(L):
        kin = I + Ic if l == 0 else H
        params += [(torch.rand(4 * H, kin, generator=g) * 2 - 1) * k * w_scale, (torch.rand(4 * H, H, generator=g) * 2 - 1) * k * wh_scale,
                   (torch.rand(4 * H, generator=g) * 2 - 1) * k * w_scale, (torch.rand(4 * H, generator=g) * 2 - 1) * k * w_scale]
    x = torch.randn(T, B, I, generator=g) * x_scale if I else None
    xc = torch.randn(B, Ic, generator=g) * x_scale if Ic else None
    return x, xc, params, torch.randn(T, B, H, generator=g), torch.randn(B, L * H, generator=g)


def _bins(shape, div):
    """Bin index of every element: each dimension's index divided by div[k]."""
    ids = torch.zeros(shape, dtype=torch.int64)
    mul = 1
    for k in reversed(range(len(shape))):
        n = -(-shape[k] // div[k])
        idx = (torch.arange(shape[k]) // div[k]).view([-1 if j == k else 1 for j in range(len(shape))])
        ids = ids + idx * mul
        mul *= n
    return ids, mul


def bin_divisors(name: str, shape) -> tuple:
    if name in ("hs_top", "hs_lp"):
        return (1, 32, 64)
    if len(shape) == 1:        # bias
        return (64,)
    if name.startswith("weight"):
        return (64, 64)
    return (32, 64)            # hn, d_xc


def measure(name: str, got: torch.Tensor, want: torch.Tensor) -> dict:
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(want.abs().max().item(), 1e-30)
    e = got - want
    a = e.abs()
    ids, n = _bins(tuple(e.shape), bin_divisors(name, e.shape))
    ids = ids.reshape(-1)
    s = torch.bincount(ids, weights=a.reshape(-1), minlength=n)
    c = torch.bincount(ids, minlength=n).double()
    bm = (s / c.clamp_min(1))[c > 0]
    med = bm.median().item()
    return {"name": name, "scale": scale, "finite": bool(torch.isfinite(got).all()), "max": a.max().item() / scale,
            "mean": a.mean().item() / scale, "signed": abs(e.mean().item()) / scale,
            "bin_max": bm.max().item() / scale, "bin_med": med / scale}


def failures(st: dict, consts: dict, kind: str) -> list:
    c = consts[kind]
    bad = []
    if not st["finite"]:
        bad.append("not finite")
    for k in ("max", "mean", "signed"):
        if not st[k] <= c[k]:
            bad.append("%s %.3g > %.3g" % (k, st[k], c[k]))
    lim = LOCAL_RATIO * st["bin_med"] + consts["floor"]
    if not st["bin_max"] <= lim:
        bad.append("local: worst bin %.3g > %.3g (median bin %.3g)" % (st["bin_max"], lim, st["bin_med"]))
    return bad


def fmt(st: dict) -> str:
    return "%-12s max %.2e mean %.2e signed %.2e bin %.2e/med %.2e (scale %.3g)" % (
        st["name"], st["max"], st["mean"], st["signed"], st["bin_max"], st["bin_med"], st["scale"])


def named_tensors(hs_top, hn, grads, d_xc, L, hs_lp=None) -> dict:
    """The tensors of one lstm_seq run under the comparator's names (None entries are left out)."""
    out = {}
    if hs_top is not None:
        out["hs_top"] = hs_top
    if hs_lp is not None:
        out["hs_lp"] = hs_lp
    if hn is not None:
        out["hn"] = hn
    for l in range(L):
        for k, n in enumerate(("weight_ih", "weight_hh", "bias_ih", "bias_hh")):
            out["%s_l%d" % (n, l)] = grads[4 * l + k]
    if d_xc is not None:
        out["d_xc"] = d_xc
    return out


def compare(got: dict, want: dict, consts: dict, label: str = "", quiet: bool = False) -> list:
    """Measure every tensor of `want` present in `got`; print what was measured; return the list of failures."""
    bad = []
    for name, w in want.items():
        if name not in got:
            continue
        st = measure(name, got[name], w)
        kind = "fwd" if name in ("hs_top", "hs_lp", "hn") else "grad"
        f = failures(st, consts, kind)
        if not quiet:
            print("%s %s%s" % (label, fmt(st), ("  FAIL: " + "; ".join(f)) if f else ""))
        bad += ["%s %s: %s" % (label, name, x) for x in f]
    return bad
