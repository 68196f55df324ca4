"""Float64 Gaussian heads (K2) and fused lower bound (K3), forward and backward written out, rounding where the kernels round.

Lower bound, per segment b (simple_fhvae.py:105-116, oracle/ref_cpu.elbo_terms):
    log_px_z   = -0.5 (T F log 2pi + sum_{t,f} lv + df^2 e^-lv),  df = x - x_mu           loss.hip:89-92, 103-122
    neg_kld_z1 = 0.5 sum_j 1 + lv - mu^2 - e^lv                                           loss.hip:126-130
    neg_kld_z2 = 0.5 sum_j 1 + lv - lv2 - ((mu - m2)^2 + e^lv) / v2                        loss.hip:131-136
    log_pmu2   = -0.5 sum_j log 2pi + m2^2                                                 loss.hip:135, 138
    lower_bound = log_px_z + neg_kld_z1 + neg_kld_z2 + log_pmu2 / num_segs                 loss.hip:141-146
lv2 = the f32 log 0.25 (loss.hip:12), v2 = its f32 exp (loss.hip:125, 180; numpy's in ref_cpu.kld).
Backward (loss.hip:150-234): the upstream gradients enter as elbo_upstream sums them (loss.hip:166-176, an absent one is 0):
    gpx = glb + g_px, gk1 = glb + g_k1, gk2 = glb + g_k2, gpm = glb / ns + g_pm
    d_x_mu = gpx df e^-lv, d_x_lv = -0.5 gpx (1 - df^2 e^-lv)                              loss.hip:150-163, 203-230
    d_z1_mu = -mu gk1, d_z1_lv = 0.5 (1 - e^lv) gk1                                        loss.hip:181-186
    d_z2_mu = -(mu - m2) / v2 gk2, d_z2_lv = 0.5 (1 - e^lv / v2) gk2                       loss.hip:187-192
    d_mu2 = (mu - m2) / v2 gk2 - m2 gpm (the prior term only without reference_detach)    loss.hip:193
  reference_detach: no d_x (loss.hip:203) and no prior term in d_mu2.
Pair form (elbo_bwd_pair_kernel, loss.hip:241-307): rows r = t B + b of [rb(d_x_mu) | rb(d_x_lv) | 0] (loss.hip:276-283)
and the column sums of the UNROUNDED f32 values (loss.hip:284-285, 297-306).

bf16 head (_GaussHeadLp, hip_binding.py; gemm.hip, proj.hip, wgrad.hip):
    operands rb(h) (the caller's h_lp), rb([W_mu; W_lv]) (head_pair_weights_kernel, gemm.hip:536-546), f32 biases;
    [mu | lv] = rb(h) rb(W)^T + b (proj.hip / gemm_kernel: exact bf16 products, f32 accumulation)
    sample = mu + eps e^{0.5 lv}                                                            gemm.hip:549-560
    g = [rb(d_mu + d_s) | rb(d_lv + d_s eps 0.5 e^{0.5 lv}) | 0]                             gemm.hip:563-590
    dh = g rb(W), dW = g^T rb(h)                                                            gemm.hip:840-895
    db = column sums of rb(g) (gemm.hip:594-604 fused, colsum_kernel gemm.hip:420-477) or, with the lower bound's partial
         rows, of its unrounded f32 gradient (add_split_kernel, gemm.hip:609-636): bias_from = "rounded" | "f32".
f32 head (_GaussHead; gemm.hip:725-762, 922-972): the same without rounding (v_mfma_f32_16x16x4_f32 counted as exact f32).
mu2 table backward (gather_bwd_kernel, loss.hip:75-83): dtable[idx - off] += scale dmu2, rows outside [0, S) skipped.

rb(v) = v.float().bfloat16().double(): round to nearest even from f32, as f2bf (common.h:34) rounds the kernels' f32 values.
Every function returns float64 tensors on its inputs' device, and with each result "a_<name>": the sum of the absolute values of
the terms that make it (the conditioning the comparator's bounds scale with; the lower bound and its gradients can cancel).
In those sums a difference x - mu counts as |x| + |mu| and e^v as e^v (1 + |v|): one f32 ulp of an input moves them that much.

`_fault` is for the comparator's own tests only (tests/test_head_elbo_oracle_cpu.py), a deliberately wrong variant:
  {"drop_step": (b, t)}       elbo: one time step missing from row b's log_px_z
  {"scalar_nsegs": n}         elbo: the scalar n used where per-row num_segs were given
  {"lv_no_half": True}        elbo backward: d_x_lv = gpx (1 - df^2 e^-lv) (the -0.5 dropped)
  {"prior_kept": True}        elbo backward: the prior term of d_mu2 kept under reference_detach
  {"drop_last_b": True}       colsum: the last segment (b = B - 1) missing
  {"pad_nonzero": True}       pair rows: the first padding column 1.0 (or, without padding, no fault)
  {"batch_major": True}       pair rows: written at r = b T + t
  {"exp_full_lv": True}       head: sample = mu + eps e^lv
  {"drop_k_tile": True}       head backward: dh without the last 64-wide tile of its 2D-long contraction
  {"drop_m_tile": True}       head backward: dW without the last 64-row tile of its M-long contraction
"""
import math
from typing import Optional

import numpy as np
import torch

LOG2PI = math.log(2 * math.pi)
LV2 = float(np.float32(np.log(0.5 ** 2)))  # kPz2Logvar, loss.hip:12
V2 = float(np.exp(np.float32(LV2)))        # expf(kPz2Logvar) (f32), loss.hip:125, 180
UPSTREAMS = ("lower_bound", "log_px_z", "neg_kld_z1", "neg_kld_z2", "log_pmu2")


def rb(v: torch.Tensor) -> torch.Tensor:
    return v.float().bfloat16().double()


def _d(t):
    return None if t is None else t.detach().double()


def _nsegs(num_segs, B, dev, fault):
    if "scalar_nsegs" in fault:
        return torch.full((B,), float(fault["scalar_nsegs"]), dtype=torch.float64, device=dev)
    if isinstance(num_segs, torch.Tensor):
        return num_segs.detach().to(dev).double()
    return torch.full((B,), float(np.float32(num_segs)), dtype=torch.float64, device=dev)  # (float)nsegs_scalar, loss.hip:140


def elbo_ref_fwd(x, x_mu, x_lv, z1_mu, z1_lv, z2_mu, z2_lv, mu2, num_segs, _fault: Optional[dict] = None) -> dict:
    """x, x_mu, x_lv batch-major (B, T, F) (the kernels' layouts are the caller's business); z*, mu2 (B, D1 / D2); num_segs an
    int64 (B,) tensor or a number (the scalar form).  Returns the five (B,) outputs and their a_* sums."""
    fault = _fault or {}
    x, xm, xl = _d(x), _d(x_mu), _d(x_lv)
    m1, l1, m2_, l2, p = _d(z1_mu), _d(z1_lv), _d(z2_mu), _d(z2_lv), _d(mu2)
    B, T, F = x.shape
    ns = _nsegs(num_segs, B, x.device, fault)
    df = x - xm
    q = df * df * torch.exp(-xl)
    qa = (x.abs() + xm.abs()) ** 2 * torch.exp(-xl) * (1.0 + xl.abs())
    term = xl + q
    if "drop_step" in fault:
        b, t = fault["drop_step"]
        term = term.clone()
        term[b, t] = 0.0
    px = -0.5 * (T * F * LOG2PI + term.sum((1, 2)))
    a_px = 0.5 * (T * F * LOG2PI + (xl.abs() + qa).sum((1, 2)))
    k1 = 0.5 * (1.0 + l1 - m1 * m1 - torch.exp(l1)).sum(1)
    a_k1 = 0.5 * (1.0 + l1.abs() + m1 * m1 + torch.exp(l1) * (1.0 + l1.abs())).sum(1)
    d2 = m2_ - p
    k2 = 0.5 * (1.0 + l2 - LV2 - (d2 * d2 + torch.exp(l2)) / V2).sum(1)
    a_k2 = 0.5 * (1.0 + l2.abs() + abs(LV2) + ((m2_.abs() + p.abs()) ** 2 + torch.exp(l2) * (1.0 + l2.abs())) / V2).sum(1)
    pm = -0.5 * (LOG2PI + p * p).sum(1)
    a_pm = 0.5 * (LOG2PI + p * p).sum(1)
    return {"lower_bound": px + k1 + k2 + pm / ns, "log_px_z": px, "neg_kld_z1": k1, "neg_kld_z2": k2, "log_pmu2": pm,
            "a_lower_bound": a_px + a_k1 + a_k2 + a_pm / ns, "a_log_px_z": a_px, "a_neg_kld_z1": a_k1, "a_neg_kld_z2": a_k2,
            "a_log_pmu2": a_pm}


def elbo_ref_bwd(x, x_mu, x_lv, z1_mu, z1_lv, z2_mu, z2_lv, mu2, num_segs, ups: dict, reference_detach: bool,
                 _fault: Optional[dict] = None) -> dict:
    """ups: upstream gradient name (UPSTREAMS) -> (B,) tensor; a missing or None entry is 0 (elbo_upstream, loss.hip:166-176).
    Returns d_x_mu, d_x_lv (B, T, F; None under reference_detach), d_z1_mu, d_z1_lv, d_z2_mu, d_z2_lv, d_mu2 and their a_*."""
    fault = _fault or {}
    x, xm, xl = _d(x), _d(x_mu), _d(x_lv)
    m1, l1, m2_, l2, p = _d(z1_mu), _d(z1_lv), _d(z2_mu), _d(z2_lv), _d(mu2)
    B = x.shape[0]
    ns = _nsegs(num_segs, B, x.device, fault)
    z = torch.zeros(B, dtype=torch.float64, device=x.device)
    u = {n: (_d(ups[n]).to(x.device) if ups.get(n) is not None else z) for n in UPSTREAMS}
    glb = u["lower_bound"]
    gpx, gk1, gk2 = glb + u["log_px_z"], glb + u["neg_kld_z1"], glb + u["neg_kld_z2"]
    gpm = glb / ns + u["log_pmu2"]
    a_gpx, a_gk1, a_gk2 = (glb.abs() + u[n].abs() for n in ("log_px_z", "neg_kld_z1", "neg_kld_z2"))
    a_gpm = glb.abs() / ns + u["log_pmu2"].abs()
    out = {}
    if reference_detach:
        out.update(d_x_mu=None, d_x_lv=None, a_d_x_mu=None, a_d_x_lv=None)
    else:
        df = x - xm
        iv = torch.exp(-xl)
        sa, iva = x.abs() + xm.abs(), iv * (1.0 + xl.abs())
        g3, a3 = gpx[:, None, None], a_gpx[:, None, None]
        out["d_x_mu"] = g3 * df * iv
        out["a_d_x_mu"] = a3 * sa * iva
        out["d_x_lv"] = (1.0 if fault.get("lv_no_half") else -0.5) * g3 * (1.0 - df * df * iv)
        out["a_d_x_lv"] = 0.5 * a3 * (1.0 + sa * sa * iva)
    out["d_z1_mu"], out["a_d_z1_mu"] = -m1 * gk1[:, None], (m1 * a_gk1[:, None]).abs()
    out["d_z1_lv"], out["a_d_z1_lv"] = 0.5 * (1.0 - torch.exp(l1)) * gk1[:, None], 0.5 * (1.0 + torch.exp(l1) * (1.0 + l1.abs())) * a_gk1[:, None]
    dd, dda = (m2_ - p) / V2, (m2_.abs() + p.abs()) / V2
    out["d_z2_mu"], out["a_d_z2_mu"] = -dd * gk2[:, None], dda * a_gk2[:, None]
    out["d_z2_lv"] = 0.5 * (1.0 - torch.exp(l2) / V2) * gk2[:, None]
    out["a_d_z2_lv"] = 0.5 * (1.0 + torch.exp(l2) * (1.0 + l2.abs()) / V2) * a_gk2[:, None]
    out["d_mu2"], out["a_d_mu2"] = dd * gk2[:, None], dda * a_gk2[:, None]
    if not reference_detach or fault.get("prior_kept"):
        out["d_mu2"] = out["d_mu2"] - p * gpm[:, None]
        out["a_d_mu2"] = out["a_d_mu2"] + (p * a_gpm[:, None]).abs()
    return out


def pair_rows(d_x_mu, d_x_lv, ld_pair: int, _fault: Optional[dict] = None) -> torch.Tensor:
    """The bf16 operand elbo_bwd_pair_kernel writes, as float64: (T B, ld_pair) rows r = t B + b of [rb(d_x_mu) | rb(d_x_lv) |
    0] (loss.hip:276-283); d_x_mu / d_x_lv batch-major (B, T, F)."""
    fault = _fault or {}
    B, T, F = d_x_mu.shape
    o = torch.zeros(B, T, ld_pair, dtype=torch.float64, device=d_x_mu.device)
    o[:, :, :F], o[:, :, F:2 * F] = rb(d_x_mu), rb(d_x_lv)
    if fault.get("pad_nonzero") and ld_pair > 2 * F:
        o[:, :, 2 * F] = 1.0
    if fault.get("batch_major"):
        return o.reshape(B * T, ld_pair)
    return o.transpose(0, 1).reshape(T * B, ld_pair)


def pair_colsum(d_x_mu, d_x_lv, a_d_x_mu=None, a_d_x_lv=None, _fault: Optional[dict] = None):
    """(sum, a_sum), each (2F,): the column sums of [d_x_mu | d_x_lv] over every (b, t) -- the unrounded values, as
    elbo_bwd_pair_kernel sums them (loss.hip:284-285) -- and the sums of their conditioning (elbo_ref_bwd's a_d_x_*, when given:
    an f32 d_x_lv that cancels carries the error of its terms, not of its value) or else of their absolute values."""
    fault = _fault or {}
    g = torch.cat([_d(d_x_mu), _d(d_x_lv)], 2)
    a = torch.cat([_d(a_d_x_mu), _d(a_d_x_lv)], 2) if a_d_x_mu is not None else g.abs()
    if fault.get("drop_last_b"):
        g = g[:-1]
    g = g.reshape(-1, g.shape[2])
    return g.sum(0), a.reshape(-1, a.shape[2]).sum(0)


def _ops(h, w_mu, w_lv, lp):
    h, w = _d(h), torch.cat([_d(w_mu), _d(w_lv)], 0)
    return (rb(h), rb(w)) if lp else (h, w)


def head_ref_fwd(h, w_mu, b_mu, w_lv, b_lv, eps=None, lp: bool = True, _fault: Optional[dict] = None) -> dict:
    """mu, lv (M, D) and, with eps, the sample; their a_* (|h| |W|^T + |b|; the sample's from the float64 mu, lv)."""
    hr, w = _ops(h, w_mu, w_lv, lp)
    D = w_mu.shape[0]
    b = torch.cat([_d(b_mu), _d(b_lv)]).to(hr.device)
    out = hr @ w.T + b
    a = hr.abs() @ w.abs().T + b.abs()
    r = {"mu": out[:, :D], "lv": out[:, D:], "a_mu": a[:, :D], "a_lv": a[:, D:]}
    if eps is not None:
        r.update(sample_ref(r["mu"], r["lv"], eps, _fault))
    return r


def sample_ref(mu, lv, eps, _fault: Optional[dict] = None) -> dict:
    """sample = mu + eps e^{0.5 lv} (gemm.hip:496-500, 549-560) of the given mu, lv (the kernel's own, chained)."""
    fault = _fault or {}
    mu, lv, e = _d(mu), _d(lv), _d(eps).to(mu.device)
    s = e * torch.exp(lv if fault.get("exp_full_lv") else 0.5 * lv)
    return {"sample": mu + s, "a_sample": mu.abs() + s.abs()}


def head_ref_g(d_mu, d_lv, d_s, eps, lv, ldg: int, lp: bool = True) -> dict:
    """g (M, ldg) = [d_mu + d_s | d_lv + d_s eps 0.5 e^{0.5 lv} | 0] unrounded ("g") and as the bf16 operand ("g_lp", lp only;
    gemm.hip:563-590), and a_g.  Any of d_mu, d_lv, d_s may be None (0)."""
    ref = next(t for t in (d_mu, d_lv, d_s) if t is not None)
    M, D = ref.shape
    dev = ref.device
    z = torch.zeros(M, D, dtype=torch.float64, device=dev)
    dm, dl, ds = (_d(t) if t is not None else z for t in (d_mu, d_lv, d_s))
    sl = ds * _d(eps).to(dev) * 0.5 * torch.exp(0.5 * _d(lv).to(dev)) if d_s is not None else z
    g = torch.zeros(M, ldg, dtype=torch.float64, device=dev)
    a = torch.zeros_like(g)
    g[:, :D], g[:, D:2 * D] = dm + ds, dl + sl
    a[:, :D], a[:, D:2 * D] = dm.abs() + ds.abs(), dl.abs() + sl.abs()
    r = {"g": g, "a_g": a}
    if lp:
        r["g_lp"] = rb(g)
    return r


def head_ref_bwd(g, h, w_mu, w_lv, lp: bool = True, _fault: Optional[dict] = None) -> dict:
    """dh = g[:, :2D] W (M, K) and dW = g[:, :2D]^T h (2D, K: dW_mu over dW_lv) from the operand g (for chained checks: the
    kernel's own g_lp), with rb(h), rb(W) in the bf16 form; and their a_* (|g| |W|, |g|^T |h|)."""
    fault = _fault or {}
    hr, w = _ops(h, w_mu, w_lv, lp)
    D2 = w.shape[0]
    g = _d(g)[:, :D2].to(hr.device)
    gk = g
    if fault.get("drop_k_tile"):
        gk = g.clone()
        gk[:, (D2 - 1) // 64 * 64:] = 0.0
    gm = g
    if fault.get("drop_m_tile"):
        gm = g.clone()
        gm[(g.shape[0] - 1) // 64 * 64:] = 0.0
    return {"dh": gk @ w, "a_dh": g.abs() @ w.abs(), "dW": gm.T @ hr, "a_dW": g.abs().T @ hr.abs()}


def head_ref_bias(g: dict, D: int, bias_from: str = "rounded") -> dict:
    """db (2D,) = column sums of head_ref_g's g: of the bf16 operand (bias_from = "rounded": the fused sums in
    reparam_bwd_pair_kernel<true> and colsum_kernel) or of the unrounded values ("f32": the lower bound's partial rows through
    add_split_kernel; and the f32 head), with a_db."""
    assert bias_from in ("rounded", "f32"), bias_from
    src = g["g_lp"] if bias_from == "rounded" else g["g"]
    return {"db": src[:, :2 * D].sum(0), "a_db": src[:, :2 * D].abs().sum(0)}


def mu2_gather_bwd_ref(dmu2, idx, idx_offset: int, S: int, scale: float = 1.0, dtable=None) -> dict:
    """dtable (S, D) (+ the given initial table) with scale * dmu2[b] added at row idx[b] - idx_offset, rows outside [0, S) skipped
    (loss.hip:75-83; scale is an f32 argument); a_dtable: the same of the absolute values."""
    dm = _d(dmu2)
    sc = float(np.float32(scale))
    loc = idx.detach().to(dm.device).long() - int(idx_offset)
    keep = (loc >= 0) & (loc < S)
    t = torch.zeros(S, dm.shape[1], dtype=torch.float64, device=dm.device)
    if dtable is not None:
        t += _d(dtable).to(dm.device)
    a = t.abs()
    t.index_add_(0, loc[keep], sc * dm[keep])
    a.index_add_(0, loc[keep], abs(sc) * dm[keep].abs())
    return {"dtable": t, "a_dtable": a}
