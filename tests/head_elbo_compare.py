"""One comparator for the Gaussian heads (K2) and the fused lower bound (K3) against the float64 oracle of their own arithmetic
(oracle/head_elbo_ref.py), with one set of constants per mode shared by every case: tests/test_head_elbo_oracle_gpu.py checks
the kernels with it, tests/test_head_elbo_oracle_cpu.py checks that it rejects the errors a kernel could hide.

Every bound scales with the element's own conditioning (the oracle's a_* sums), not with the tensor maximum, in units of
U = 2^-24 (one f32 rounding):
  contraction   r_ij = |err_ij| / (U sqrt(K) (|A| |B|)_ij + floor)     dh (K = 2D), dW (K = M), mu | lv (K = the head's K)
  elementwise   r_i  = |err_i| / (U a_i + floor)                          the lower bound's five terms (a_i = the row's sum of
                                                                          absolute terms), its gradients, the sample
  bias sums     r_n  = |err_n| / (U sum_m |g_mn| + floor)                 (no sqrt(M): at M = 40960 a sum of the wrong source --
                                                                          rounded vs f32 g, ~2^-9 sqrt(M) |g| -- would hide under
                                                                          it; the kernels' blocked f32 sums stay far below)
Each check bounds the max and the mean of r, |mean of the signed ratio| (a bias the max would allow; from SIGN_MIN elements), and the worst bin's mean
r against LOCAL_RATIO x the median bin's + a floor: 64 x 64 output tiles of dh and dW (the last partial tiles included), rows and
time steps of the lower bound's d_x.  An error confined to one tile, row or step stands out there long before the max moves.
bf16 outputs against rb(reference): at most one bf16 ulp on at most ULP_FRAC of the elements; padding exactly 0.  g_lp's reference
is the oracle's g; d_x_pair_lp's is the kernel's own f32 d_x (chained: where d_x_lv cancels, its f32 value is good to its terms'
size, not its own, and rb of it may sit many ulps from rb(oracle); the f32 d_x itself is checked against the oracle).

Chaining: each downstream check takes the kernel's own rounded intermediate (dh and dW the kernel's g_lp, the sample the
kernel's mu and lv, d_x_pair_lp the kernel's f32 d_x), so a single ulp flip upstream cannot force loose bounds downstream.  The
end-to-end checks through the autograd binding chain the same way: the kernel's own bf16 operand is reproduced by the same
deterministic launch on the same inputs, so they keep the per-mode constants.
"""
import math

import torch

U = 2.0 ** -24
LOCAL_RATIO = 8.0
ULP_FRAC = 1e-3
SIGN_MIN = 1024  # the signed mean is judged from this many elements on (a handful of rows is no statistic)

# Measured.  The floor (test_head_elbo_oracle_cpu.py::test_noise_floor_is_below_the_constants: the oracle against itself, the
# f32 inputs moved by one ulp; c2's decoder shapes, the four regimes): lower bound terms and gradients max 5.2 / mean 0.91; f32
# head contractions max 0.089 / mean 0.012 (mu, lv, dh, dW), bf16 mu, lv 2.7e-3 (dh, dW chained: 0); sample max 4.9 / mean 0.72;
# bias sums max 0.93 / mean 0.16.
# The kernels on an MI355X (test_head_elbo_oracle_gpu.py, every case): lower bound max 4.6 (the pair kernel's d_x_lv) / mean 0.79;
# bf16 head contractions max 0.51 (dh) / mean 0.012; f32 head max 1.05 (dh) / mean 0.096; sample, g_ws max 3.0 / mean 0.38;
# g_lp at most 1 ulp on <= 2.3e-5 of the elements, d_x_pair_lp bit-exact (chained); bias sums and mu2_gather_bwd max 2.7 / mean 0.83;
# no bin above LOCAL_RATIO x its median.  The constants sit above both; the faults of the CPU file land 30x and more above them.
ELBO = {"max": 16.0, "mean": 2.0, "sign": 0.5, "bin": 2.0}
HEAD = {
    "bf16": {"cmax": 4.0, "cmean": 0.5, "csign": 0.2, "cbin": 0.5, "emax": 16.0, "emean": 2.0, "esign": 0.5, "ebin": 1.0,
             "bmax": 8.0, "bmean": 2.0},
    "f32": {"cmax": 8.0, "cmean": 1.0, "csign": 0.3, "cbin": 1.0, "emax": 16.0, "emean": 2.0, "esign": 0.5, "ebin": 1.0,
            "bmax": 8.0, "bmean": 2.0},
}


def _bins(r: torch.Tensor, ids: torch.Tensor):
    ids = ids.reshape(-1).long()
    n = int(ids.max().item()) + 1
    s = torch.bincount(ids, weights=r.reshape(-1), minlength=n)
    k = torch.bincount(ids, minlength=n).double()
    bm = (s / k.clamp_min(1))[k > 0]
    return bm.max().item(), bm.median().item()


def tile_ids(shape, tile=64) -> torch.Tensor:
    R, C = shape
    nc = -(-C // tile)
    return (torch.arange(R)[:, None] // tile) * nc + torch.arange(C)[None, :] // tile


def measure(got, want, den, bins=()) -> dict:
    """r = |got - want| / den and its statistics; bins: (name, ids) pairs (ids shaped like got)."""
    want = want.double()
    got = got.detach().to(want.device).double()
    assert got.shape == want.shape, (got.shape, want.shape)
    den = den.to(want.device)
    err = got - want
    r = err.abs() / den
    fin = bool(torch.isfinite(got).all())
    r = torch.nan_to_num(r, nan=1e30, posinf=1e30)
    st = {"finite": fin, "n": r.numel(), "max": r.max().item(), "mean": r.mean().item(), "sign": (err / den).mean().item(), "bins": {}}
    for name, ids in bins:
        st["bins"][name] = _bins(r, ids.to(r.device).expand_as(r))
    return st


def failures(st: dict, mx: float, mean: float, sign: float, binf: float) -> list:
    bad = [] if st["finite"] else ["not finite"]
    if not st["max"] <= mx:
        bad.append("max %.3g > %.3g" % (st["max"], mx))
    if not st["mean"] <= mean:
        bad.append("mean %.3g > %.3g" % (st["mean"], mean))
    if st["n"] >= SIGN_MIN and not abs(st["sign"]) <= sign:
        bad.append("signed mean %.3g > %.3g" % (st["sign"], sign))
    for n, (bmax, bmed) in st["bins"].items():
        lim = LOCAL_RATIO * bmed + binf
        if not bmax <= lim:
            bad.append("%s bins: worst %.3g > %.3g (median %.3g)" % (n, bmax, lim, bmed))
    return bad


def fmt(st: dict) -> str:
    b = " ".join("%s %.2e/%.2e" % (n, a, m) for n, (a, m) in st["bins"].items())
    return "max %.2e mean %.2e sign %+.1e %s" % (st["max"], st["mean"], st["sign"], b)


def _report(label, st, bad, quiet, log):
    if log is not None:
        log.append((label, st))
    if not quiet:
        print("%-40s %s%s" % (label, fmt(st), ("  FAIL: " + "; ".join(bad)) if bad else ""))
    return ["%s: %s" % (label, b) for b in bad]


def _floor(a: torch.Tensor, scale: float) -> float:
    return 1e-30 + 1e-7 * scale * a.abs().max().item()


def check_contraction(got, want, a, K: int, k: dict, label="", quiet=False, log=None) -> list:
    """A contraction of length K (mu | lv, dh, dW): 64 x 64 tile bins."""
    a = a.double()
    den = U * math.sqrt(K) * a + _floor(a, U * math.sqrt(K))
    st = measure(got, want, den, (("tile", tile_ids(tuple(want.shape))),))
    return _report(label, st, failures(st, k["cmax"], k["cmean"], k["csign"], k["cbin"]), quiet, log)


def check_elementwise(got, want, a, k: dict, label="", quiet=False, log=None, bins=()) -> list:
    """Elementwise f32 arithmetic (the sample, the lower bound's terms and gradients); k: ELBO or a HEAD mode's e*."""
    a = a.double()
    den = U * a + _floor(a, U)
    st = measure(got, want, den, bins)
    kk = k if "max" in k else {"max": k["emax"], "mean": k["emean"], "sign": k["esign"], "bin": k["ebin"]}
    return _report(label, st, failures(st, kk["max"], kk["mean"], kk["sign"], kk["bin"]), quiet, log)


def check_bias(got, want, a, k: dict, label="", quiet=False, log=None) -> list:
    """Column sums (the bias gradients, the lower bound's column sums): a = sum of |g| per column."""
    a = a.double()
    den = U * a + _floor(a, U)
    st = measure(got, want, den)
    return _report(label, st, failures(st, k["bmax"], k["bmean"], k["bmax"], 0.0), quiet, log)


def row_time_bins(B: int, T: int, F: int):
    """Bins of a batch-major (B, T, F) gradient: per row and per time step."""
    b = torch.arange(B)[:, None, None].expand(B, T, F)
    t = torch.arange(T)[None, :, None].expand(B, T, F)
    return (("row", b), ("step", t))


def bf16_keys(v: torch.Tensor) -> torch.Tensor:
    """Ordered integer keys of bf16 values (adjacent bf16 numbers differ by 1; +0 and -0 are both 0)."""
    u = v.detach().to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF
    mag = u & 0x7FFF
    return torch.where(u >= 0x8000, -mag, mag)


def check_bf16(got_lp, want, n_data: int, label="", quiet=False, log=None) -> list:
    """got_lp (R, ld) bf16 from the kernel; want (R, ld) float64, unrounded oracle values in columns [0, n_data) (zeros after).
    At most one ulp from rb(want), on at most ULP_FRAC of the data elements; the padding columns exactly +0."""
    got = got_lp.detach().to(want.device)
    assert got.shape == want.shape and got.dtype == torch.bfloat16, (got.shape, got.dtype, want.shape)
    d = (bf16_keys(got[:, :n_data]) - bf16_keys(want[:, :n_data].float())).abs()
    pad = got[:, n_data:].view(torch.int16)
    st = {"max_ulp": int(d.max().item()), "frac": (d > 0).double().mean().item(), "pad_nonzero": int((pad != 0).sum().item())}
    bad = []
    if st["max_ulp"] > 1:
        bad.append("max %d ulp" % st["max_ulp"])
    if st["frac"] > ULP_FRAC:
        bad.append("%.2e of the elements off by an ulp > %.0e" % (st["frac"], ULP_FRAC))
    if st["pad_nonzero"]:
        bad.append("%d padding elements not +0" % st["pad_nonzero"])
    if log is not None:
        log.append((label, st))
    if not quiet:
        print("%-40s ulp max %d frac %.2e pad %d%s" % (label, st["max_ulp"], st["frac"], st["pad_nonzero"],
                                                     ("  FAIL: " + "; ".join(bad)) if bad else ""))
    return ["%s: %s" % (label, b) for b in bad]


# ---------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------
REGIMES = ("typical", "lv_neg", "lv_pos", "prior")


def elbo_inputs(B: int, T: int, F: int, D1: int, D2: int, regime: str, seed: int) -> dict:
    """Seeded CPU f32 inputs of the lower bound, batch-major (B, T, F).
    typical: x, x_mu N(0,1), x_lv 0.5 N(0,1), latents N(0,1), lv 0.5 N(0,1);  lv_neg: x_lv = -8 + 0.3 N(0,1) (e^-lv amplifies
    |x - mu|);  lv_pos: x_lv = 6 + 0.3 N(0,1);  prior: posteriors at the priors (z1 N(0,1e-6), lv 1e-3 N; z2 = mu2 + 1e-3 N, lv =
    log 0.25 + 1e-3 N: the KL terms near 0, where only the floor and the sums of absolute terms apply).  num_segs 1..200."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)
    x, xm = n(B, T, F), n(B, T, F)
    xl = {"lv_neg": -8.0 + 0.3 * n(B, T, F), "lv_pos": 6.0 + 0.3 * n(B, T, F)}.get(regime, 0.5 * n(B, T, F))
    mu2 = n(B, D2)
    if regime == "prior":
        z1m, z1l = 1e-3 * n(B, D1), 1e-3 * n(B, D1)
        z2m, z2l = mu2 + 1e-3 * n(B, D2), math.log(0.25) + 1e-3 * n(B, D2)
    else:
        z1m, z1l, z2m, z2l = n(B, D1), 0.5 * n(B, D1), n(B, D2), 0.5 * n(B, D2)
    ns = torch.randint(1, 200, (B,), generator=g)
    ups = {k: n(B) for k in ("lower_bound", "log_px_z", "neg_kld_z1", "neg_kld_z2", "log_pmu2")}
    return {"x": x, "x_mu": xm, "x_lv": xl, "z": [z1m, z1l, z2m, z2l, mu2], "num_segs": ns, "ups": ups}


def head_inputs(M: int, K: int, D: int, seed: int, sample: bool = True) -> dict:
    """Seeded CPU f32 inputs of a head: h N(0,1), W 0.05 N(0,1) (nn.Linear-like), b 0.1 N; upstream d_mu, d_lv, d_s N(0,1);
    eps N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)
    return {"h": n(M, K), "w_mu": 0.05 * n(D, K), "b_mu": 0.1 * n(D), "w_lv": 0.05 * n(D, K), "b_lv": 0.1 * n(D),
            "eps": n(M, D) if sample else None, "d_mu": n(M, D), "d_lv": n(M, D), "d_s": n(M, D) if sample else None}
