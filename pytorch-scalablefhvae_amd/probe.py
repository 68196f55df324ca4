"""probe.py -- frame probes ("Frame probes"): a multinomial logistic regression (softmax regression) trained on
frame-level representations to predict a frame's phone or its speaker, the supervised check beside ABX, units and posteriorgrams.

  table, rows, gradient    the bindings of include/fhvae_probe.h (csrc/probe.hip): the model as the device table; every row's
                   log-sum-exp, arg-max class and negative log-likelihood with their float64 totals; the (C, W + 1) float64
                   gradient of the summed negative log-likelihood, with no (N, C) array
  objective        the mean negative log-likelihood plus the L2 penalty, and its gradient, on float64 host parameters
  minimise, fit    L-BFGS with a backtracking line search; the fit from zero parameters
  score            accuracy, balanced accuracy, loss and the confusion table of a fitted model
  frame_labels, split_utterances   a label per frame from an item file; a seeded utterance split
  save / load      one .npz: weights (C, D), bias (C,), mean (D,), std (D,), classes (C,), float64

A model is a dict of float64 numpy arrays "weights", "bias", "mean", "std", "classes": the logit of class c on a raw row x is
bias[c] + weights[c] . ((x - mean) / std).  The definitions (the order of the sums, the stop rule) are this project's, written
out in include/fhvae_probe.h and below; nothing here runs scikit-learn.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

import hip_ext

#: include/fhvae_probe.h, FHVAE_PROBE_*
PROBE_SLICE = 1024
PROBE_MAX_W = 128
PROBE_MAX_ROWS, PROBE_MAX_CLASSES = 1 << 30, 1 << 16
NOUN = "the probe"  # (in the messages of hip_ext's checks)

_vp, _i64 = C.c_void_p, C.c_int64
#: the entry points of include/fhvae_probe.h: name -> (restype, argtypes).  Exported from libfhvae_hip.so but not part of
#: include/fhvae_hip.h (ABI 12 is unchanged), so they are bound from this table (hip_ext.load) and not in hip_binding.SIGNATURES
PROBE_SIGNATURES = {
    "fhvae_probe_ws_bytes": (_i64, [_i64, _i64, _i64]),
    "fhvae_probe_rows": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "fhvae_probe_grad": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
}


def load_library():
    """hip_binding.load_library() with the probe entry points bound (argtypes from PROBE_SIGNATURES)."""
    return hip_ext.load(PROBE_SIGNATURES)


def padded(width):
    """W: the width rounded up to a multiple of 16."""
    return (int(width) + 15) // 16 * 16


def ws_bytes(N, n_classes, W):
    """fhvae_probe_ws_bytes without the library: the f32 partials (slices, C, W + 1) and the float64 partials (slices, 3), each
    rounded up to 256 bytes."""
    slices = -(-int(N) // PROBE_SLICE)
    return (slices * int(n_classes) * (int(W) + 1) * 4 + 255) // 256 * 256 + (slices * 24 + 255) // 256 * 256


# ---------------------------------------------------------------------------------------------------------------- raw calls
def _rows(op, name, t):
    """The (N, D) f32 rows of a call -> (rows (N, W), D): a device tensor with dense rows; a width that is no multiple of 16 is
    zero-padded on the device (every value of the header is unchanged), so is a view the kernels cannot take as it is."""
    return hip_ext.padded_rows(op, name, t, NOUN, 16, PROBE_MAX_W, PROBE_MAX_ROWS)


def _device(op, name, t, dtype, shape):
    return hip_ext.device_tensor(op, name, t, NOUN, dtype, shape=shape, contiguous=True)


def _labels(op, y, N, n_classes):
    """y (N,) integers on the device -> int32, its largest value below n_classes (one host sync; a negative value is
    'unlabelled')."""
    import torch

    hip_ext.device_tensor(op, "y", y, NOUN)
    if y.dim() != 1 or int(y.shape[0]) != N or y.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("%s: y must be (%d,) int32 or int64 (got %s %s)" % (op, N, y.dtype, tuple(y.shape)))
    top = int(y.max())
    if top >= n_classes:
        raise RuntimeError("%s: y holds class %d, the table has %d classes" % (op, top, n_classes))
    return y.to(torch.int32).contiguous()


def table(weights, bias, mean=None, std=None, device=None):
    """The model as the kernels read it (include/fhvae_probe.h) -> (tab (C, W) f32, cst (C,) f32), in float64 on the device and
    rounded once, with the column standardisation folded in so that raw rows go in:
        tab[c][d] = weights[c][d] / std[d]        cst[c] = bias[c] - sum_d weights[c][d] mean[d] / std[d]"""
    import torch

    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("table: the probe runs on a MI355X only (no CPU fallback)")
        device = torch.device("cuda", torch.cuda.current_device())
    w = torch.as_tensor(weights, dtype=torch.float64).to(device)
    b = torch.as_tensor(bias, dtype=torch.float64).to(device)
    if w.dim() != 2 or b.dim() != 1 or b.shape[0] != w.shape[0] or w.shape[0] < 1 or w.shape[1] < 1:
        raise RuntimeError("table: weights %s and bias %s are no (C, D), (C,)" % (tuple(w.shape), tuple(b.shape)))
    n_classes, D = int(w.shape[0]), int(w.shape[1])
    if D > PROBE_MAX_W or n_classes > PROBE_MAX_CLASSES:
        raise RuntimeError("table: %d classes of %d columns, the probe kernels take at most %d of %d" % (n_classes, D, PROBE_MAX_CLASSES, PROBE_MAX_W))
    mu = torch.zeros(D, dtype=torch.float64, device=device) if mean is None else torch.as_tensor(mean, dtype=torch.float64).to(device)
    sd = torch.ones(D, dtype=torch.float64, device=device) if std is None else torch.as_tensor(std, dtype=torch.float64).to(device)
    if tuple(mu.shape) != (D,) or tuple(sd.shape) != (D,) or not bool((sd > 0).all()):
        raise RuntimeError("table: mean and std must be (%d,), std positive" % D)
    tab = torch.zeros(n_classes, padded(D), dtype=torch.float64, device=device)
    tab[:, :D] = w / sd[None, :]
    cst = b - (tab[:, :D] * mu[None, :]).sum(dim=1)
    return tab.float().contiguous(), cst.float().contiguous()


def _pass_args(op, x, y, tab, cst):
    import torch

    x, D = _rows(op, "x", x)
    W = int(x.shape[1])
    if tab is None or not isinstance(tab, torch.Tensor) or tab.dim() != 2:
        raise RuntimeError("%s: tab must be the 2-D table of probe.table" % op)
    n_classes = int(tab.shape[0])
    _device(op, "tab", tab, torch.float32, (n_classes, W))
    _device(op, "cst", cst, torch.float32, (n_classes,))
    y = _labels(op, y, int(x.shape[0]), n_classes)
    return x, y, W, n_classes


def _workspace(op, dev, N, n_classes, W):
    need = int(load_library().fhvae_probe_ws_bytes(N, n_classes, W))
    if need <= 0:
        raise RuntimeError("%s: %d rows / %d classes / %d columns lie outside the kernels' limits (%d rows, %d classes)"
                           % (op, N, n_classes, W, PROBE_MAX_ROWS, PROBE_MAX_CLASSES))
    return hip_ext.workspace("probe", dev, need)


def _enqueue_rows(x, y, tab, cst, W, n_classes, totals):
    import torch

    import hip_binding as hb

    N = int(x.shape[0])
    lse = torch.empty(N, dtype=torch.float32, device=x.device)
    pred = torch.empty(N, dtype=torch.int32, device=x.device)
    nll = torch.empty(N, dtype=torch.float32, device=x.device)
    ws = _workspace("rows", x.device, N, n_classes, W)
    hb._call("fhvae_probe_rows", hb._p(x), x.stride(0), N, W, hb._p(tab), tab.stride(0), hb._p(cst), n_classes, hb._p(y), hb._p(lse),
             hb._p(pred), hb._p(nll), hb._p(totals), hb._p(ws), ws.numel())
    return lse, pred, nll


def _enqueue_grad(x, y, tab, cst, W, n_classes, lse, grad):
    import hip_binding as hb

    N = int(x.shape[0])
    ws = _workspace("gradient", x.device, N, n_classes, W)
    hb._call("fhvae_probe_grad", hb._p(x), x.stride(0), N, W, hb._p(tab), tab.stride(0), hb._p(cst), n_classes, hb._p(y), hb._p(lse),
             hb._p(grad), hb._p(ws), ws.numel())


def rows(x, y, tab, cst):
    """fhvae_probe_rows.  x (N, D) f32 and y (N,) integers on the device (a negative y: unlabelled), (tab, cst) of table() ->
    (lse (N,) f32, pred (N,) int32, nll (N,) f32, totals (3,) float64: sum nll, labelled rows, labelled rows with pred == y).
    Only enqueues (after the check of y's largest value)."""
    import torch

    load_library()
    x, y, W, n_classes = _pass_args("rows", x, y, tab, cst)
    totals = torch.empty(3, dtype=torch.float64, device=x.device)
    lse, pred, nll = _enqueue_rows(x, y, tab, cst, W, n_classes, totals)
    return lse, pred, nll, totals


def gradient(x, y, tab, cst, lse):
    """fhvae_probe_grad.  lse (N,) f32 as rows() returned it -> grad (C, W + 1) float64 on the device, W = D rounded up to a
    multiple of 16: grad[c] = sum over the labelled rows of (softmax - onehot)(n, c) [x[n], 1]; the bias column is the last one,
    the padding columns before it are 0.  No (N, C) array is formed.  Only enqueues."""
    import torch

    load_library()
    x, y, W, n_classes = _pass_args("gradient", x, y, tab, cst)
    _device("gradient", "lse", lse, torch.float32, (int(x.shape[0]),))
    grad = torch.empty(n_classes, W + 1, dtype=torch.float64, device=x.device)
    _enqueue_grad(x, y, tab, cst, W, n_classes, lse, grad)
    return grad


# ---------------------------------------------------------------------------------------------------------------- objective
def _host_objective(total_nll, labelled, G, params, l2, mean, std):
    """The objective and its gradient from the device's sums: G (C, D + 1) = sum r [x_raw, 1] (bias column last)."""
    D = params.shape[1] - 1
    w = params[:, :D]
    if labelled == 0:
        return 0.0, np.zeros_like(params)
    value = total_nll / labelled + 0.5 * l2 * float(np.sum(w * w))
    grad = np.empty_like(params)
    # the chain rule through z = (x - mean) / std: sum r z[d] = (sum r x[d] - mean[d] sum r) / std[d]
    grad[:, :D] = (G[:, :D] - mean[None, :] * G[:, D:]) / std[None, :] / labelled + l2 * w
    grad[:, D] = G[:, D] / labelled
    return float(value), grad


def _prepared(x, y, n_classes):
    x, D = _rows("objective", "x", x)
    y = _labels("objective", y, int(x.shape[0]), n_classes)
    return x, y, D


def _objective_prepared(x, y, D, params, l2, mean, std):
    """objective() on rows and labels that _prepared returned: two enqueued passes and ONE host sync."""
    import torch

    load_library()
    params = np.asarray(params, dtype=np.float64)
    n_classes, W = params.shape[0], int(x.shape[1])
    tab, cst = table(params[:, :D], params[:, D], mean, std, device=x.device)
    out = torch.empty(3 + n_classes * (W + 1), dtype=torch.float64, device=x.device)
    lse, _, _ = _enqueue_rows(x, y, tab, cst, W, n_classes, out[:3])
    _enqueue_grad(x, y, tab, cst, W, n_classes, lse, out[3:])
    host = out.cpu().numpy()  # the one sync
    G = host[3:].reshape(n_classes, W + 1)
    return _host_objective(float(host[0]), float(host[1]), np.concatenate([G[:, :D], G[:, W:]], axis=1), params, float(l2), mean, std)


def objective(x, y, params, l2, mean=None, std=None):
    """x (N, D) f32 and y (N,) on the device, params (C, D + 1) float64 on the host (weights, then the bias, in the standardised
    coordinates z = (x - mean) / std; mean 0 and std 1 by default) -> (value, gradient (C, D + 1) float64):
        value = mean nll over the labelled rows + l2 / 2 * ||weights||^2      (the bias is not penalised)
    One host sync per evaluation.  Without a labelled row: (0, zeros)."""
    params = np.asarray(params, dtype=np.float64)
    if params.ndim != 2 or params.shape[1] < 2:
        raise RuntimeError("objective: params must be (C, D + 1) float64")
    x, y, D = _prepared(x, y, params.shape[0])
    if params.shape[1] != D + 1:
        raise RuntimeError("objective: params has %d columns, the rows %d (+ 1 for the bias)" % (params.shape[1], D))
    mean = np.zeros(D) if mean is None else np.asarray(mean, dtype=np.float64)
    std = np.ones(D) if std is None else np.asarray(std, dtype=np.float64)
    return _objective_prepared(x, y, D, params, l2, mean, std)


# ---------------------------------------------------------------------------------------------------------------- optimiser
def minimise(fun, p0, iters=200, gtol=1e-5, memory=10, c1=1e-4, max_halvings=40):
    """L-BFGS (two-loop recursion over the last `memory` pairs) with a backtracking line search on the Armijo condition
    f(p + t d) <= f(p) + c1 t g.d, t = 1, 1/2, 1/4 ... (the first iteration starts from t = 1 / max(1, ||g||_inf)).  fun(p) ->
    (value, gradient) on float64 numpy arrays.  Stops when the infinity norm of the gradient is <= gtol, after `iters` iterations,
    or when no step of the line search lowers the objective (the rounding of fun has been reached).  A pair with s.y <= 0 is not
    stored.  Plain numpy in a fixed order: the same fun gives the same bits.
    -> (p, {"objective": [f per iteration, the start first], "iterations", "converged", "evaluations", "gradient_norm"})"""
    p = np.array(p0, dtype=np.float64)
    f, g = fun(p)
    evals = 1
    hist = {"objective": [float(f)], "iterations": 0, "converged": False, "evaluations": 1, "gradient_norm": float(np.max(np.abs(g))) if g.size else 0.0}
    S, Y = [], []
    for it in range(1, int(iters) + 1):
        gn = float(np.max(np.abs(g))) if g.size else 0.0
        if gn <= gtol:
            hist["converged"] = True
            break
        q = g.copy()
        alphas = []
        for s, yv in zip(reversed(S), reversed(Y)):
            a = float(np.sum(s * q)) / float(np.sum(s * yv))
            alphas.append(a)
            q -= a * yv
        if S:
            q *= float(np.sum(S[-1] * Y[-1])) / float(np.sum(Y[-1] * Y[-1]))
        for (s, yv), a in zip(zip(S, Y), reversed(alphas)):
            b = float(np.sum(yv * q)) / float(np.sum(s * yv))
            q += (a - b) * s
        d = -q
        slope = float(np.sum(g * d))
        if not slope < 0:  # (not a descent direction: start again from the gradient)
            S, Y, d = [], [], -g
            slope = float(np.sum(g * d))
        t = 1.0 if S else 1.0 / max(1.0, gn)
        found = False
        for _ in range(int(max_halvings)):
            pn = p + t * d
            fn, gnew = fun(pn)
            evals += 1
            if math.isfinite(fn) and fn <= f + c1 * t * slope:
                found = True
                break
            t *= 0.5
        hist["evaluations"] = evals
        if not found:
            break
        s, yv = pn - p, gnew - g
        if float(np.sum(s * yv)) > 1e-300:
            S.append(s), Y.append(yv)
            if len(S) > memory:
                S.pop(0), Y.pop(0)
        p, f, g = pn, fn, gnew
        hist["objective"].append(float(f))
        hist["iterations"] = it
    gn = float(np.max(np.abs(g))) if g.size else 0.0
    hist["gradient_norm"] = gn
    if gn <= gtol:
        hist["converged"] = True
    return p, hist


def fit(x, y, n_classes, l2=1e-4, iters=200, gtol=1e-5, standardise=True, strict=False):
    """Softmax regression on the rows of x ((N, D) f32 on the device) with labels y ((N,) integers on the device, negative:
    unlabelled), by minimise() on objective() from zero parameters.

    standardise: mean and std are the float64 column mean and standard deviation (mean((x - mean)^2)^(1/2)) of the labelled
    rows, computed on the device; a column that holds one value only gets std 1.  A class below n_classes without a training
    row keeps weights 0 and gets bias -inf (it is never predicted and adds nothing to any sum); strict=True refuses it.
    Same input: the same bits.

    -> (model: float64 numpy "weights" (C, D), "bias" (C,), "mean" (D,), "std" (D,), "classes" (C,) = 0 .. C - 1;
        history: {"objective": [per iteration, the start first], "iterations", "converged", "evaluations", "gradient_norm"})"""
    import torch

    n_classes = int(n_classes)
    if n_classes < 1 or n_classes > PROBE_MAX_CLASSES:
        raise ValueError("fit: n_classes = %d must lie in [1, %d]" % (n_classes, PROBE_MAX_CLASSES))
    if iters < 0 or not l2 >= 0:
        raise ValueError("fit: iters = %r and l2 = %r must not be negative" % (iters, l2))
    x, y, D = _prepared(x, y, n_classes)
    lab = y >= 0
    counts = torch.bincount(y[lab].long(), minlength=n_classes).cpu().numpy()
    if int(counts.sum()) == 0:
        raise ValueError("fit: no row has a label")
    if strict and not counts.all():
        raise ValueError("fit: class %d has no training row" % int(np.nonzero(counts == 0)[0][0]))
    if not bool(torch.isfinite(x[lab]).all()):
        raise ValueError("fit: x holds values that are not finite")
    if standardise:
        xd = x[lab][:, :D].double()
        mu = xd.mean(dim=0)
        sd = ((xd - mu[None, :]) ** 2).mean(dim=0).sqrt()
        mean, std = mu.cpu().numpy(), sd.cpu().numpy()
        std = np.where(std > 0, std, 1.0)
    else:
        mean, std = np.zeros(D), np.ones(D)
    # a class without a training row is no variable: weights 0 and bias -inf (probability 0, gradient 0), the others from 0
    present = counts > 0
    params = np.zeros((n_classes, D + 1))
    params[~present, D] = -np.inf

    def fun(q):
        params[present] = q
        value, grad = _objective_prepared(x, y, D, params, l2, mean, std)
        return value, grad[present]

    q, hist = minimise(fun, np.zeros((int(present.sum()), D + 1)), iters, gtol)
    params[present] = q
    model = {"weights": params[:, :D].copy(), "bias": params[:, D].copy(), "mean": mean, "std": std,
             "classes": np.arange(n_classes, dtype=np.float64)}
    return model, hist


def _model_arrays(op, model):
    try:
        w, b, mean, std, classes = (np.asarray(model[k], dtype=np.float64) for k in ("weights", "bias", "mean", "std", "classes"))
    except (KeyError, TypeError):
        raise ValueError("%s: a model is a dict of weights, bias, mean, std and classes" % op) from None
    if w.ndim != 2 or b.shape != (w.shape[0],) or mean.shape != (w.shape[1],) or std.shape != mean.shape or classes.shape != b.shape:
        raise ValueError("%s: weights %s, bias %s, mean %s, std %s, classes %s are no (C, D), (C,), (D,), (D,), (C,)"
                         % (op, w.shape, b.shape, mean.shape, std.shape, classes.shape))
    return w, b, mean, std, classes


def confusion(y, pred, n_classes):
    """The (C, C) float64 table n[truth][prediction] of the frames with y >= 0, by np.add.at (as units.unit_quality)."""
    y, pred = np.asarray(y).astype(np.int64), np.asarray(pred).astype(np.int64)
    keep = y >= 0
    tab = np.zeros((int(n_classes), int(n_classes)), dtype=np.float64)
    np.add.at(tab, (y[keep], pred[keep]), 1.0)
    return tab


def summarise(conf, total_nll):
    """accuracy, balanced_accuracy (the mean recall over the classes present), loss (nats per frame), frames of a confusion
    table and the summed nll."""
    n = float(conf.sum())
    if n == 0:
        return {"accuracy": 0.0, "balanced_accuracy": 0.0, "loss": 0.0, "frames": 0, "confusion": conf}
    per = conf.sum(axis=1)
    here = per > 0
    return {"accuracy": float(np.trace(conf) / n), "balanced_accuracy": float(np.mean(np.diag(conf)[here] / per[here])),
            "loss": float(total_nll) / n, "frames": int(n), "confusion": conf}


def score(x, y, model):
    """x (N, D) f32 and y (N,) on the device, a model of fit() or load() -> {"accuracy", "balanced_accuracy", "loss", "frames",
    "confusion" (C, C) float64: n[truth][prediction]} over the labelled rows."""
    w, b, mean, std, _ = _model_arrays("score", model)
    tab, cst = table(w, b, mean, std, device=x.device if hasattr(x, "device") and x.is_cuda else None)
    _, pred, _, totals = rows(x, y, tab, cst)
    return summarise(confusion(y.cpu().numpy(), pred.cpu().numpy(), w.shape[0]), float(totals[0]))


# ------------------------------------------------------------------------------------------------------------------- labels
def frame_labels(items, keys, lengths, column="phone", frame_shift=0.010, frame_offset=0.0):
    """Item lines (abx.read_items) -> a label per frame: units.frame_phones on the phone column, or the same rule on the
    speaker column.  -> (labels (total frames,) int32, -1 where no token lies; names in order of first use; overlaps)."""
    import units

    if column == "phone":
        return units.frame_phones(items, keys, lengths, frame_shift, frame_offset)
    if column != "speaker":
        raise ValueError("frame_labels: column %r is neither 'phone' nor 'speaker'" % (column,))
    swapped = [(name, on, off, speaker, prev, nxt, speaker) for name, on, off, _, prev, nxt, speaker in items]
    return units.frame_phones(swapped, keys, lengths, frame_shift, frame_offset)


def split_utterances(n_utts, holdout, seed=0):
    """-> (train, test): utterance indices, sorted.  RandomState(seed).permutation(n_utts), of which the last
    ceil(holdout * n_utts) are the test set.  ValueError unless both sides get an utterance."""
    n_utts = int(n_utts)
    if not 0.0 < float(holdout) < 1.0:
        raise ValueError("split_utterances: holdout %r must lie in (0, 1)" % (holdout,))
    n_test = int(math.ceil(float(holdout) * n_utts))
    if n_utts < 2 or n_test < 1 or n_test >= n_utts:
        raise ValueError("split_utterances: %d utterance(s) with holdout %g leave no train or no test utterance" % (n_utts, holdout))
    perm = np.random.RandomState(int(seed)).permutation(n_utts)
    return np.sort(perm[:n_utts - n_test]), np.sort(perm[n_utts - n_test:])


def frames_of(utts, lengths):
    """The frame indices of the utterances `utts` in a corpus whose utterances lie one after the other."""
    lengths = np.asarray(lengths, dtype=np.int64)
    base = np.concatenate([[0], np.cumsum(lengths)])
    return np.concatenate([np.arange(base[u], base[u + 1]) for u in utts]) if len(utts) else np.zeros(0, np.int64)


def majority(train_y, test_y, n_classes):
    """The test accuracy of always answering the most frequent training class (the smallest index of equal counts)."""
    train_y, test_y = np.asarray(train_y), np.asarray(test_y)
    counts = np.bincount(train_y[train_y >= 0], minlength=int(n_classes))
    test = test_y[test_y >= 0]
    return float(np.mean(test == int(np.argmax(counts)))) if test.size else 0.0


def run(train_x, train_y, test_x, test_y, names, l2=1e-4, iters=200, gtol=1e-5, model=None):
    """What both command lines do with a split: fit on the training rows (or take `model`), score both sides.
    -> (model, report: the keys of probe.json but on / target / unlabelled / overlaps, confusion (C, C) of the test side)."""
    import torch

    n_classes = len(names)
    hist = {"iterations": 0, "converged": True}
    if model is None:
        model, hist = fit(train_x, train_y, n_classes, l2=l2, iters=iters, gtol=gtol)
    elif _model_arrays("run", model)[0].shape != (n_classes, int(train_x.shape[1])):
        raise ValueError("the model has weights %s, the data %d classes of %d columns" % (model["weights"].shape, n_classes, train_x.shape[1]))
    test, train = score(test_x, test_y, model), score(train_x, train_y, model)
    ty, sy = train_y.cpu().numpy(), test_y.cpu().numpy()
    report = {"classes": list(names), "train_frames": train["frames"], "test_frames": test["frames"], "accuracy": test["accuracy"],
              "balanced_accuracy": test["balanced_accuracy"], "majority": majority(ty, sy, n_classes), "train_accuracy": train["accuracy"],
              "loss": test["loss"], "iterations": int(hist["iterations"]), "converged": bool(hist["converged"]), "l2": float(l2)}
    return model, report, test["confusion"]


# --------------------------------------------------------------------------------------------------------------------- files
KEYS = ("weights", "bias", "mean", "std", "classes")


def save(path, model):
    """One .npz with weights (C, D), bias (C,), mean (D,), std (D,), classes (C,), float64."""
    arrays = dict(zip(KEYS, (np.ascontiguousarray(a) for a in _model_arrays("save", model))))
    with open(path, "wb") as fh:  # (np.savez would add ".npz" to a name without it)
        np.savez(fh, **arrays)


def load(path):
    """The inverse of save: a model of numpy float64 arrays, its shapes checked."""
    with np.load(path) as z:
        try:
            model = {key: np.asarray(z[key], dtype=np.float64) for key in KEYS}
        except KeyError as e:
            raise ValueError("%s holds no %s: not a file probe.save wrote" % (path, e)) from None
    _model_arrays(path, model)
    return model
