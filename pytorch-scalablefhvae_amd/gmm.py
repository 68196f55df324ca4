"""gmm.py -- soft acoustic units from frame-level representations ("GMM"): a diagonal-covariance Gaussian mixture
fitted on the rows of a corpus by EM, and the per-frame posteriors over its components (the posteriorgram).

  table, loglik, posteriors, accumulate   the bindings of include/fhvae_gmm.h (csrc/gmm.hip): the model as the device table;
                   every row's log-likelihood and arg-max component; its posteriors; the sufficient statistics nk, sx, sxx
  chunk_rows       how the rows of a corpus are cut so that the (rows, K) posteriors and the workspace fit a byte budget
  estep, mstep     an EM iteration on those: the float64 statistics of all rows, and the model they give
  fit              EM from a k-means start (units.fit)
  posteriorgram    (N, K) f32 posteriors of a fitted model
  save / load      one .npz: weights (K,), means (K, D), variances (K, D), float64

A model is a dict of float64 "weights" (K,), "means" (K, D), "variances" (K, D): torch tensors on the device inside fit, numpy
arrays on disk; table() takes either.  The definitions (the table, the order of the sums, the floors, the stop rule) are this
project's, written out in include/fhvae_gmm.h and below; nothing here runs scikit-learn or Kaldi.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

import hip_ext

#: include/fhvae_gmm.h, FHVAE_GMM_*
GMM_SLICE = 1024
GMM_MAX_DP = 64
GMM_MAX_ROWS, GMM_MAX_COMP = 1 << 30, 1 << 20

_vp, _i64 = C.c_void_p, C.c_int64
#: the entry points of include/fhvae_gmm.h: name -> (restype, argtypes).  Exported from libfhvae_hip.so but not part of
#: include/fhvae_hip.h (ABI 12 is unchanged), so they are bound from this table (hip_ext.load) and not in hip_binding.SIGNATURES
GMM_SIGNATURES = {
    "fhvae_gmm_ws_bytes": (_i64, [_i64, _i64, _i64]),
    "fhvae_gmm_loglik": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    "fhvae_gmm_post": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp]),
    "fhvae_gmm_stats": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, C.c_int, _vp]),
}


def load_library():
    """hip_binding.load_library() with the mixture entry points bound (argtypes from GMM_SIGNATURES)."""
    return hip_ext.load(GMM_SIGNATURES)


def padded(width):
    """Dp: the width rounded up to a multiple of 8."""
    return (int(width) + 7) // 8 * 8


def ws_bytes(N, K, Dp):
    """fhvae_gmm_ws_bytes without the library: the f32 partials (slices, K, 2 Dp + 1), rounded up to 256 bytes."""
    return (-(-int(N) // GMM_SLICE) * int(K) * (2 * int(Dp) + 1) * 4 + 255) // 256 * 256


# ---------------------------------------------------------------------------------------------------------------- raw calls
def _rows(op, name, t):
    """The (N, D) f32 rows of a call -> (rows (N, Dp), D): a device tensor with dense rows; a width that is no multiple of 8 is
    zero-padded on the device (every value of the header is unchanged), so is a view the kernels cannot take as it is."""
    return hip_ext.padded_rows(op, name, t, "the mixture", 8, GMM_MAX_DP, GMM_MAX_ROWS)


def _device_f32(op, name, t, shape):
    import torch

    hip_ext.device_tensor(op, name, t, "the mixture")
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):  # (this module's wording: "float32", not "torch.float32")
        raise RuntimeError("%s: %s must be float32 of shape %s (got %s %s)" % (op, name, tuple(shape), t.dtype, tuple(t.shape)))
    return t


def _model_arrays(op, model):
    """weights, means, variances of a model as float64 torch tensors (where they are), checked."""
    import torch

    try:
        w, mu, var = (torch.as_tensor(model[key]) for key in ("weights", "means", "variances"))
    except (KeyError, TypeError):
        raise RuntimeError("%s: a model is a dict of weights, means and variances" % op) from None
    if w.dtype != torch.float64 or mu.dtype != torch.float64 or var.dtype != torch.float64:
        raise RuntimeError("%s: the model's weights, means and variances are float64" % op)
    if w.dim() != 1 or mu.dim() != 2 or tuple(var.shape) != tuple(mu.shape) or mu.shape[0] != w.shape[0] or w.shape[0] < 1:
        raise RuntimeError("%s: weights %s, means %s, variances %s are no (K,), (K, D), (K, D)" % (op, tuple(w.shape), tuple(mu.shape), tuple(var.shape)))
    if mu.shape[1] < 1 or mu.shape[1] > GMM_MAX_DP:
        raise RuntimeError("%s: the model has %d columns, the mixture kernels take 1 to %d" % (op, mu.shape[1], GMM_MAX_DP))
    if w.shape[0] > GMM_MAX_COMP:
        raise RuntimeError("%s: the model has %d components, the mixture kernels take at most %d" % (op, w.shape[0], GMM_MAX_COMP))
    if not bool((w >= 0).all()) or not bool((w > 0).any()):
        raise RuntimeError("%s: the model's weights must be non-negative and not all 0" % op)
    if not bool((var > 0).all()) or not bool(torch.isfinite(var).all()) or not bool(torch.isfinite(mu).all()):
        raise RuntimeError("%s: the model's variances must be positive and its means finite" % op)
    return w, mu, var


def table(model, device=None):
    """The model as the kernels read it (include/fhvae_gmm.h) -> (tab (K, 2 Dp) f32, cst (K,) f32), built in float64 on the
    device and rounded once.  A model whose weights are all 0 is refused."""
    import torch

    w, mu, var = _model_arrays("table", model)
    if device is None:
        device = w.device if w.is_cuda else None
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("table: the mixture runs on a MI355X only (no CPU fallback)")
        device = torch.device("cuda", torch.cuda.current_device())
    w, mu, var = w.to(device), mu.to(device), var.to(device)
    K, D = int(mu.shape[0]), int(mu.shape[1])
    Dp = padded(D)
    tab = torch.zeros(K, 2 * Dp, dtype=torch.float64, device=device)
    tab[:, :D] = mu / var
    tab[:, Dp:Dp + D] = -1.0 / (2.0 * var)
    cst = torch.log(w) - (D * math.log(2.0 * math.pi) + torch.log(var).sum(dim=1) + (mu * mu / var).sum(dim=1)) / 2.0
    return tab.float().contiguous(), cst.float().contiguous()


def _pass_args(op, x, tab, cst):
    import torch

    x, D = _rows(op, "x", x)
    Dp = int(x.shape[1])
    if tab is None or not isinstance(tab, torch.Tensor) or tab.dim() != 2:
        raise RuntimeError("%s: tab must be the 2-D table of gmm.table" % op)
    K = int(tab.shape[0])
    _device_f32(op, "tab", tab, (K, 2 * Dp))
    _device_f32(op, "cst", cst, (K,))
    if not tab.is_contiguous() or not cst.is_contiguous():
        raise RuntimeError("%s: tab and cst must be contiguous (as gmm.table returns them)" % op)
    return x, Dp, K


def loglik(x, tab, cst):
    """fhvae_gmm_loglik.  x (N, D) f32 on the device, (tab, cst) of table() -> (loglik (N,) f32, labels (N,) int32): every row's
    log-likelihood under the mixture and its arg-max component (equal values: the smallest index).  Only enqueues."""
    import torch

    import hip_binding as hb

    load_library()
    x, Dp, K = _pass_args("loglik", x, tab, cst)
    N = int(x.shape[0])
    ll = torch.empty(N, dtype=torch.float32, device=x.device)
    labels = torch.empty(N, dtype=torch.int32, device=x.device)
    hb._call("fhvae_gmm_loglik", hb._p(x), x.stride(0), N, Dp, hb._p(tab), tab.stride(0), hb._p(cst), K, hb._p(ll), hb._p(labels))
    return ll, labels


def posteriors(x, tab, cst, loglik, out=None):
    """fhvae_gmm_post.  loglik (N,) f32 as loglik() returned it -> post (N, K) f32 = expf(l - loglik): a view of an allocation
    whose rows are padded to a multiple of 4, or `out` ((N, K) f32 on the device, dense rows, a row stride that is a multiple
    of 4, a 16-byte aligned start).  Only enqueues."""
    import torch

    import hip_binding as hb

    load_library()
    x, Dp, K = _pass_args("posteriors", x, tab, cst)
    N = int(x.shape[0])
    _device_f32("posteriors", "loglik", loglik, (N,))
    if not loglik.is_contiguous():
        raise RuntimeError("posteriors: loglik must be contiguous")
    if out is None:
        out = torch.empty(N, (K + 3) // 4 * 4, dtype=torch.float32, device=x.device)[:, :K]
    _post_rows("posteriors", "out", out, N, K)
    hb._call("fhvae_gmm_post", hb._p(x), x.stride(0), N, Dp, hb._p(tab), tab.stride(0), hb._p(cst), K, hb._p(loglik), hb._p(out),
             out.stride(0))
    return out


def _post_rows(op, name, t, N, K):
    _device_f32(op, name, t, (N, K))
    if not hip_ext.rows_dense(t, K):
        raise RuntimeError("%s: %s needs dense rows, a row stride that is a multiple of 4 and a 16-byte aligned start (strides %s)"
                           % (op, name, tuple(t.stride())))


def _workspace(dev, N, K, Dp):
    need = int(load_library().fhvae_gmm_ws_bytes(N, K, Dp))
    if need <= 0:
        raise RuntimeError("accumulate: %d rows / %d components / %d columns lie outside the kernels' limits (%d rows, %d components)"
                           % (N, K, Dp, GMM_MAX_ROWS, GMM_MAX_COMP))
    return hip_ext.workspace("gmm", dev, need)


def accumulate(x, post, stats=None):
    """fhvae_gmm_stats.  x (N, D), post (N, K) f32 on the device -> {"nk" (K,), "sx" (K, Dp), "sxx" (K, Dp)} float64 on the
    device (Dp: D rounded up to a multiple of 8; the padding columns are 0).  With `stats` (what an earlier call returned) the
    sums are added onto it, in place: over row chunks cut at multiples of GMM_SLICE that equals one call bit for bit.  Only
    enqueues."""
    import torch

    import hip_binding as hb

    load_library()
    x, D = _rows("accumulate", "x", x)
    N, Dp = int(x.shape[0]), int(x.shape[1])
    if post is None or not isinstance(post, torch.Tensor) or post.dim() != 2:
        raise RuntimeError("accumulate: post must be a 2-D device tensor")
    K = int(post.shape[1])
    _post_rows("accumulate", "post", post, N, K)
    if stats is None:
        out = {"nk": torch.empty(K, dtype=torch.float64, device=x.device), "sx": torch.empty(K, Dp, dtype=torch.float64, device=x.device),
               "sxx": torch.empty(K, Dp, dtype=torch.float64, device=x.device)}
    else:
        out = stats
        for key, shape in (("nk", (K,)), ("sx", (K, Dp)), ("sxx", (K, Dp))):
            t = out.get(key)
            if t is None or not t.is_cuda or t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous():
                raise RuntimeError("accumulate: stats[%r] must be a contiguous float64 device tensor of shape %s" % (key, shape))
    ws = _workspace(x.device, N, K, Dp)
    hb._call("fhvae_gmm_stats", hb._p(x), x.stride(0), N, Dp, hb._p(post), post.stride(0), K, hb._p(ws), ws.numel(), hb._p(out["nk"]),
             hb._p(out["sx"]), hb._p(out["sxx"]), 0 if stats is None else 1)
    return out


# ----------------------------------------------------------------------------------------------------------------------- EM
def chunk_rows(N, K, width, max_bytes=512 << 20):
    """The row counts estep walks a corpus in: every chunk but the last the same multiple of GMM_SLICE, the largest whose
    (rows, K rounded up to 4) f32 posteriors plus fhvae_gmm_ws_bytes stay within max_bytes.  A function of its arguments alone.
    ValueError if one slice does not fit."""
    N, K, Dp = int(N), int(K), padded(width)
    if N < 1 or K < 1:
        raise ValueError("chunk_rows: N = %d and K = %d must be at least 1" % (N, K))
    ldp = (K + 3) // 4 * 4
    per_slice = GMM_SLICE * ldp * 4 + K * (2 * Dp + 1) * 4
    slices = int(max_bytes) // per_slice
    if slices >= 1 and slices * GMM_SLICE * ldp * 4 + ws_bytes(slices * GMM_SLICE, K, Dp) > max_bytes:
        slices -= 1  # (the workspace is rounded up to 256 bytes, less than a slice takes)
    if slices < 1:
        raise ValueError("chunk_rows: %d bytes hold no slice of %d rows at K = %d (%d bytes)"
                         % (max_bytes, GMM_SLICE, K, GMM_SLICE * ldp * 4 + ws_bytes(GMM_SLICE, K, Dp)))
    chunk = slices * GMM_SLICE
    return [chunk] * (N // chunk) + ([N % chunk] if N % chunk else [])


def estep(x, model, max_bytes=512 << 20):
    """The E-step over all rows of x ((N, D) f32 on the device) in the chunks of chunk_rows: per chunk loglik, posteriors into
    one reused buffer, accumulate onto the running statistics.  -> (stats {"nk" (K,), "sx" (K, D), "sxx" (K, D)} float64 on
    the device, the float64 sum of loglik (a 0-d device tensor: no host sync), labels (N,) int32).  The chunks depend on
    (N, K, D, max_bytes) alone, so two runs give the same bits."""
    import torch

    tab, cst = table(model, x.device if isinstance(x, torch.Tensor) and x.is_cuda else None)
    x, D = _rows("estep", "x", x)
    N, K = int(x.shape[0]), int(tab.shape[0])
    if int(tab.shape[1]) != 2 * int(x.shape[1]):
        raise RuntimeError("estep: the rows have %d columns, the model %d" % (D, int(np.shape(model["means"])[1])))
    chunks = chunk_rows(N, K, D, max_bytes)
    buf = torch.empty(chunks[0], (K + 3) // 4 * 4, dtype=torch.float32, device=x.device)
    labels = torch.empty(N, dtype=torch.int32, device=x.device)
    total = torch.zeros((), dtype=torch.float64, device=x.device)
    stats, a = None, 0
    for c in chunks:
        xc = x[a:a + c]
        ll, labels[a:a + c] = loglik(xc, tab, cst)
        post = posteriors(xc, tab, cst, ll, out=buf[:c, :K])
        stats = accumulate(xc, post, stats)
        total = total + ll.double().sum()
        a += c
    return {"nk": stats["nk"], "sx": stats["sx"][:, :D], "sxx": stats["sxx"][:, :D]}, total, labels


def mstep(stats, prev, n, global_var, var_floor=0.01, min_count=3.0):
    """The model of the statistics, in float64 torch ops (on whatever device they are):
        w = nk / n     mu = sx / nk     var = max(sxx / nk - mu^2, var_floor * global_var[d])
    A component with nk < min_count keeps prev's mean and variance (its weight is still nk / n) and is counted as starved.
    -> (model, starved, floored: the variance entries of the other components that the floor raised)."""
    import torch

    nk, sx, sxx = (torch.as_tensor(stats[key]) for key in ("nk", "sx", "sxx"))
    pmu, pvar = torch.as_tensor(prev["means"]).to(nk.device), torch.as_tensor(prev["variances"]).to(nk.device)
    floor = float(var_floor) * torch.as_tensor(global_var, dtype=torch.float64).to(nk.device)
    ok = (nk >= float(min_count))[:, None]
    safe = torch.where(ok[:, 0], nk, torch.ones_like(nk))[:, None]
    mu = sx / safe
    raw = sxx / safe - mu * mu
    low = ok & (raw < floor[None, :])
    var = torch.maximum(raw, floor[None, :].expand_as(raw))
    model = {"weights": nk / float(n), "means": torch.where(ok, mu, pmu), "variances": torch.where(ok, var, pvar)}
    return model, int((~ok).sum()), int(low.sum())


def global_variance(x):
    """The per-column variance of all rows in float64 on the device: mean((x - mean)^2)."""
    xd = x.double()
    return ((xd - xd.mean(dim=0, keepdim=True)) ** 2).mean(dim=0)


def fit(x, k, iters=50, tol=1e-4, seed=0, var_floor=0.01, kmeans_iters=10, init=None, max_bytes=512 << 20):
    """EM on the rows of x ((N, D) f32 on the device).

    The start is `init` (a model) or: the means are the centroids of units.fit(x, k, iters=kmeans_iters, seed=seed), the weights
    its counts over N (a cluster without rows starts at weight 0 and stays there), every variance the global per-column
    variance (a column that holds one value only is refused: ValueError).  An iteration
    is estep (the mean log-likelihood of the CURRENT model goes into the history), then the stop rule, then mstep: it stops
    BEFORE the M-step when the mean log-likelihood rose by less than tol times its magnitude over the iteration before, so the
    model returned is then the one the last history entry belongs to; after `iters` iterations the last M-step's model is
    returned.  Same input and seed: the same bits.

    -> (model: float64 "weights", "means", "variances" on the device; history: {"mean_loglik": [per iteration], "iterations",
    "converged", "starved", "floored" (of the last M-step)})."""
    import torch

    import units

    rows = x  # (estep pads a width that is no multiple of 8 itself)
    x, D = _rows("fit", "x", x)
    N, k = int(x.shape[0]), int(k)
    if iters < 1:
        raise ValueError("fit: iters = %d must be at least 1" % iters)
    if not bool(torch.isfinite(x).all()):
        raise ValueError("fit: x holds values that are not finite")
    gvar = global_variance(x[:, :D])
    if not bool((gvar > 0).all()):
        raise ValueError("fit: column %d of x holds one value only: its variance has no floor" % int(torch.nonzero(~(gvar > 0))[0]))
    if init is not None:
        w, mu, var = _model_arrays("fit", init)
        if tuple(mu.shape) != (k, D):
            raise ValueError("fit: init has means %s, not (%d, %d)" % (tuple(mu.shape), k, D))
        model = {"weights": w.to(x.device).clone(), "means": mu.to(x.device).clone(), "variances": var.to(x.device).clone()}
    else:
        if k < 1 or k > N:
            raise ValueError("fit: k = %d must lie in [1, N = %d]" % (k, N))
        wide = int(x.shape[1])
        xk = x if wide % 16 == 0 else torch.nn.functional.pad(x, (0, 16 - wide % 16))
        km = units.fit(xk.contiguous(), k, iters=int(kmeans_iters), seed=int(seed))
        model = {"weights": torch.from_numpy(km["counts"].astype(np.float64)).to(x.device) / float(N),
                 "means": km["centroids"][:, :D].double(),
                 "variances": gvar[None, :].repeat(k, 1)}
    hist = {"mean_loglik": [], "iterations": 0, "converged": False, "starved": 0, "floored": 0}
    prev = None
    for it in range(1, int(iters) + 1):
        stats, total, _ = estep(rows, model, max_bytes)
        mean_ll = float(total) / N
        hist["mean_loglik"].append(mean_ll)
        hist["iterations"] = it
        if not math.isfinite(mean_ll):
            raise ValueError("fit: the mean log-likelihood of iteration %d is %r" % (it, mean_ll))
        if prev is not None and mean_ll - prev < tol * abs(prev):
            hist["converged"] = True
            break
        prev = mean_ll
        model, hist["starved"], hist["floored"] = mstep(stats, model, N, gvar, var_floor)
    return model, hist


def posteriorgram(x, model, max_bytes=512 << 20, with_labels=False):
    """(N, K) f32 posteriors of the rows of x under `model`, computed in the chunks of chunk_rows (a row's values do not depend
    on its chunk).  with_labels: -> (post, labels (N,) int32: the arg-max components, loglik (N,) f32)."""
    import torch

    tab, cst = table(model, x.device if isinstance(x, torch.Tensor) and x.is_cuda else None)
    x, D = _rows("posteriorgram", "x", x)
    N, K = int(x.shape[0]), int(tab.shape[0])
    if int(tab.shape[1]) != 2 * int(x.shape[1]):
        raise RuntimeError("posteriorgram: the rows have %d columns, the model %d" % (D, int(np.shape(model["means"])[1])))
    post = torch.empty(N, (K + 3) // 4 * 4, dtype=torch.float32, device=x.device)[:, :K]
    ll = torch.empty(N, dtype=torch.float32, device=x.device)
    labels = torch.empty(N, dtype=torch.int32, device=x.device)
    a = 0
    for c in chunk_rows(N, K, D, max_bytes):
        ll[a:a + c], labels[a:a + c] = loglik(x[a:a + c], tab, cst)
        posteriors(x[a:a + c], tab, cst, ll[a:a + c], out=post[a:a + c])
        a += c
    return (post, labels, ll) if with_labels else post


# --------------------------------------------------------------------------------------------------------------------- files
def save(path, model):
    """One .npz with weights (K,), means (K, D), variances (K, D), float64."""
    arrays = {}
    for key in ("weights", "means", "variances"):
        v = model[key]
        arrays[key] = np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float64)
    with open(path, "wb") as fh:  # (np.savez would add ".npz" to a name without it)
        np.savez(fh, **arrays)


def load(path):
    """The inverse of save: a model of numpy float64 arrays, its shapes checked."""
    with np.load(path) as z:
        try:
            model = {key: np.asarray(z[key], dtype=np.float64) for key in ("weights", "means", "variances")}
        except KeyError as e:
            raise ValueError("%s holds no %s: not a file gmm.save wrote" % (path, e)) from None
    w, mu, var = model["weights"], model["means"], model["variances"]
    if w.ndim != 1 or mu.ndim != 2 or var.shape != mu.shape or mu.shape[0] != w.shape[0]:
        raise ValueError("%s: weights %s, means %s, variances %s are no (K,), (K, D), (K, D)" % (path, w.shape, mu.shape, var.shape))
    return model
