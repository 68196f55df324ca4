"""ctc.py -- connectionist temporal classification on frame-level representations: the linear model of the frame
probe trained from transcriptions alone (the token order, no times) by summing over all alignments, for the corpora that ship
no time-aligned item file.

  loss             the binding of include/fhvae_ctc.h (csrc/ctc.hip): every utterance's negative log-likelihood and, if wanted,
                   its gradient with respect to the logits, by one forward-backward pass per utterance
  splice           rows with `context` neighbours per side appended, the edge frames replicated within an utterance
  objective        the mean negative log-likelihood per frame plus the L2 penalty, and its gradient, on float64 host parameters
  fit              probe.minimise on objective, from zero or from a frame-probe model; the blank is class n_phones
  greedy           arg-max per row, runs merged, the blank dropped
  recognise        fit on the training transcriptions, decode the test utterances greedily, align, phone error rate
  save / load      the probe's .npz keys plus blank and context

A model is a probe model (probe.py) with C = n_phones + 1 rows, the last one the blank's, and two more entries "blank" and
"context".  The definitions are this project's, written out in include/fhvae_ctc.h and below.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import hip_ext
from probe import _host_objective  # (the frame probe's, with the frames of the utterances used in place of its labelled rows)

#: include/fhvae_ctc.h
CTC_MAX_CLASSES = 128
CTC_MAX_LABELS = 256
CTC_BAD_PTR, CTC_BAD_LABEL, CTC_INFEASIBLE = 1, 2, 4

_vp, _i64 = C.c_void_p, C.c_int64
#: the entry points of include/fhvae_ctc.h: name -> (restype, argtypes).  Exported from libfhvae_hip.so but not part of
#: include/fhvae_hip.h (ABI 12 is unchanged), so they are bound from this table (hip_ext.load) and not in hip_binding.SIGNATURES
CTC_SIGNATURES = {
    "fhvae_ctc_ws_bytes": (_i64, [_i64]),
    "fhvae_ctc_loss": (C.c_int, [_vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
}


def load_library():
    """hip_binding.load_library() with the entry points of include/fhvae_ctc.h bound (argtypes from CTC_SIGNATURES)."""
    return hip_ext.load(CTC_SIGNATURES)


# ----------------------------------------------------------------------------------------------------------------- raw call
def _device(op, name, t, dtype, dim):
    return hip_ext.device_tensor(op, name, t, "the CTC pass", dtype, dim)


def cells(utt_ptr, lab_ptr):
    """The float64 alpha cells every utterance needs: T_u (2 L_u + 1); an utterance the kernel refuses (L_u above 256) needs none."""
    T, L = np.diff(np.asarray(utt_ptr, dtype=np.int64)), np.diff(np.asarray(lab_ptr, dtype=np.int64))
    return np.where(L > CTC_MAX_LABELS, 0, T * (2 * L + 1))


def _plan(op, utt_ptr, lab_ptr, device, want_grad, ws_limit):
    """hip_ext.BatchPlan of a batch: groups whose float64 alpha cells fit ws_limit bytes; without the gradient one group."""
    return hip_ext.BatchPlan(op, utt_ptr, lab_ptr, device, cells, 8, ws_limit if want_grad else None)


def _enqueue(lib, plan, logits, n_classes, labels, blank, nll, grad, status):
    """Every group of the plan, enqueued; nothing is read back."""
    import torch

    import hip_binding as hb

    dev = logits.device
    ws = None
    if grad is not None:
        need = int(lib.fhvae_ctc_ws_bytes(plan.ws_cells))
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    ld = (n_classes + 3) // 4 * 4
    no_rows = torch.zeros(2, ld, dtype=torch.float32, device=dev)  # (an empty array has no address)
    no_label = torch.zeros(1, dtype=torch.int32, device=dev)
    for a, b, ptrs in plan.parts:
        f0, f1, l0, l1 = int(plan.utt[a]), int(plan.utt[b]), int(plan.lab[a]), int(plan.lab[b])
        z = logits[f0:f1] if f1 > f0 else no_rows[:1]
        lab = labels[l0:l1] if l1 > l0 else no_label
        g = None
        if grad is not None:
            g = grad[f0:f1] if f1 > f0 else no_rows[1:]
        hb._call("fhvae_ctc_loss", hb._p(z), z.stride(0), f1 - f0, n_classes, blank, hb._p(ptrs[0]), hb._p(lab), hb._p(ptrs[1]),
                 hb._p(ptrs[2]) if g is not None else None, b - a, hb._p(nll[a:b]), hb._p(g) if g is not None else None,
                 g.stride(0) if g is not None else 0, hb._p(status), hb._p(ws) if g is not None else None,
                 ws.numel() if g is not None else 0)


def loss(logits, utt_ptr, labels, lab_ptr, blank, want_grad=True, ws_limit=1 << 30):
    """fhvae_ctc_loss.  logits (N, C) f32, utt_ptr (U + 1,) int64, labels int32, lab_ptr (U + 1,) int64, all on the device ->
    (nll (U,) float64, grad (N, C) f32 or None, status: the OR of CTC_BAD_LABEL and CTC_INFEASIBLE over the utterances).
    The rows are given a leading dimension that is a multiple of 4 (grad is a view of such rows).  The utterances are split into
    consecutive groups whose float64 alpha rows fit ws_limit bytes (one larger than the limit goes alone); an utterance's result
    is a function of its rows and labels alone, so the split changes no bit.  The pointers are copied to the host to plan the
    groups and the status word is read at the end: that read is the call's one wait for the kernels."""
    import torch

    op = "loss"
    logits = _device(op, "logits", logits, torch.float32, 2)
    _device(op, "utt_ptr", utt_ptr, torch.int64, 1)
    labels = _device(op, "labels", labels, torch.int32, 1).contiguous()
    _device(op, "lab_ptr", lab_ptr, torch.int64, 1)
    n_classes, blank = int(logits.shape[1]), int(blank)
    logits = hip_ext.class_rows(op, logits, "the CTC kernel", CTC_MAX_CLASSES)
    if not 0 <= blank < n_classes:
        raise RuntimeError("%s: blank = %d lies outside the %d classes" % (op, blank, n_classes))
    plan = _plan(op, utt_ptr, lab_ptr, logits.device, want_grad, ws_limit)
    N = int(logits.shape[0])
    if plan.utt[-1] != N or plan.lab[-1] > labels.shape[0]:
        raise RuntimeError("%s: the pointers end at %d rows and %d labels, the arrays hold %d and %d"
                           % (op, plan.utt[-1], plan.lab[-1], N, labels.shape[0]))
    lib = load_library()
    dev = logits.device
    nll = torch.empty(plan.U, dtype=torch.float64, device=dev)
    grad = torch.empty(N, (n_classes + 3) // 4 * 4, dtype=torch.float32, device=dev) if want_grad else None
    if plan.U == 0:
        return nll, (grad[:, :n_classes] if want_grad else None), 0
    status = hip_ext.status_word(dev)
    _enqueue(lib, plan, logits, n_classes, labels, blank, nll, grad, status)
    bits = int(status.item())
    if bits & CTC_BAD_PTR:
        raise RuntimeError("%s: the kernel refused the pointer arrays (nothing was written)" % op)
    return nll, (grad[:, :n_classes] if want_grad else None), bits


# ------------------------------------------------------------------------------------------------------------------- splice
def splice(x, utt_ptr, context):
    """x (N, D), utt_ptr (U + 1,) int64 on the same device -> (N, (2 context + 1) D): row t of an utterance becomes
    [x[t - context], .., x[t], .., x[t + context]] with the indices clamped to the utterance (its edge frames are replicated).
    Torch ops; context 0 returns x."""
    import torch

    context = int(context)
    if context < 0:
        raise ValueError("splice: context = %d must not be negative" % context)
    if context == 0 or x.shape[0] == 0:
        return x if context == 0 else x.new_zeros(0, (2 * context + 1) * x.shape[1])
    N = int(x.shape[0])
    ptr = torch.as_tensor(utt_ptr, dtype=torch.int64).to(x.device)
    rows = torch.arange(N, device=x.device)
    u = torch.searchsorted(ptr[1:].contiguous(), rows, right=True)  # the utterance of every row (empty ones are passed over)
    lo, hi = ptr[u], ptr[u + 1] - 1
    cols = [x[torch.minimum(torch.maximum(rows + k, lo), hi)] for k in range(-context, context + 1)]
    return torch.cat(cols, dim=1).contiguous()


# ---------------------------------------------------------------------------------------------------------------- objective
class _Prepared:
    """Rows, labels and the plan of a training set, built once per fit."""

    def __init__(self, op, x, utt_ptr, labels, lab_ptr, ws_limit=1 << 30):
        import torch

        self.x = _device(op, "x", x, torch.float32, 2).contiguous()
        self.labels = _device(op, "labels", labels, torch.int32, 1).contiguous()
        self.plan = _plan(op, utt_ptr, lab_ptr, x.device, True, ws_limit)
        if self.plan.utt[-1] != x.shape[0] or self.plan.lab[-1] > self.labels.shape[0]:
            raise RuntimeError("%s: the pointers end at %d rows and %d labels, the arrays hold %d and %d"
                               % (op, self.plan.utt[-1], self.plan.lab[-1], x.shape[0], self.labels.shape[0]))


def logits_of(x, tab, cst, n_cols, chunk=65536):
    """x (N, D) f32, (tab, cst) of probe.table -> x @ tab[:, :D].T + cst as (N, n_cols) f32 rows (columns past C are 0), in row
    chunks as phonerec.emissions."""
    import torch

    N, D, n_classes = int(x.shape[0]), int(x.shape[1]), int(tab.shape[0])
    out = torch.zeros(N, n_cols, dtype=torch.float32, device=x.device)
    wt = tab[:, :D].T.contiguous()
    for a in range(0, N, int(chunk)):
        out[a:a + chunk, :n_classes] = x[a:a + chunk] @ wt + cst[None, :]
    return out


def _objective_prepared(prep, params, blank, l2, mean, std, chunk=65536):
    """objective() on a _Prepared set: the logits, the CTC pass and the float64 sums are enqueued; ONE host sync."""
    import torch

    import probe

    lib = load_library()
    params = np.asarray(params, dtype=np.float64)
    x, plan = prep.x, prep.plan
    N, D, n_classes = int(x.shape[0]), int(x.shape[1]), int(params.shape[0])
    dev = x.device
    tab, cst = probe.table(params[:, :D], params[:, D], mean, std, device=dev)
    ld = (n_classes + 3) // 4 * 4
    z = logits_of(x, tab, cst, ld, chunk)
    nll = torch.empty(plan.U, dtype=torch.float64, device=dev)
    r = torch.empty(N, ld, dtype=torch.float32, device=dev)
    status = hip_ext.status_word(dev)
    if plan.U:
        _enqueue(lib, plan, z, n_classes, prep.labels, int(blank), nll, r, status)
    out = torch.zeros(2 + n_classes * (D + 1), dtype=torch.float64, device=dev)
    out[0] = nll.sum()
    out[1] = status[0].double()
    G = out[2:].view(n_classes, D + 1)
    for a in range(0, N, int(chunk)):
        rd = r[a:a + chunk, :n_classes].double()
        G[:, :D] += rd.T @ x[a:a + chunk].double()
        G[:, D] += rd.sum(dim=0)
    host = out.cpu().numpy()  # the one sync
    bits = int(host[1])
    if bits & CTC_BAD_PTR:
        raise RuntimeError("objective: the kernel refused the pointer arrays")
    if bits & CTC_BAD_LABEL:
        raise RuntimeError("objective: a transcription holds a label outside the classes, the blank, or more than %d labels" % CTC_MAX_LABELS)
    value, grad = _host_objective(float(host[0]), float(N), host[2:].reshape(n_classes, D + 1), params, float(l2), mean, std)
    return value, grad, bits


def objective(x, utt_ptr, labels, lab_ptr, params, l2, mean=None, std=None, blank=None):
    """x (N, D) f32, labels int32 on the device, utt_ptr / lab_ptr (U + 1,) (device tensors or host arrays), params (C, D + 1)
    float64 on the host (weights, then the bias, in the standardised coordinates z = (x - mean) / std, as probe.objective;
    the blank is class `blank`, by default the last) -> (value, gradient (C, D + 1) float64):
        value = sum_u nll[u] / N + l2 / 2 * ||weights||^2        (N: the frames of the utterances given; the bias is not penalised)
    The logits are x @ tab.T + cst with probe.table's (tab, cst); the gradient comes from G = sum over rows of r (x) [x, 1]
    accumulated in float64, r the kernel's gradient rows.  An utterance without an alignment makes the value +inf.
    One host sync per evaluation once the pointers are on the host."""
    params = np.asarray(params, dtype=np.float64)
    if params.ndim != 2 or params.shape[1] < 2 or params.shape[0] < 2:
        raise RuntimeError("objective: params must be (C, D + 1) float64 with C >= 2")
    prep = _Prepared("objective", x, utt_ptr, labels, lab_ptr)
    D = int(prep.x.shape[1])
    if params.shape[1] != D + 1:
        raise RuntimeError("objective: params has %d columns, the rows %d (+ 1 for the bias)" % (params.shape[1], D))
    mean = np.zeros(D) if mean is None else np.asarray(mean, dtype=np.float64)
    std = np.ones(D) if std is None else np.asarray(std, dtype=np.float64)
    blank = params.shape[0] - 1 if blank is None else int(blank)
    return _objective_prepared(prep, params, blank, l2, mean, std)[:2]


# ---------------------------------------------------------------------------------------------------------------------- fit
def feasible(length, ref):
    """Whether a transcription has an alignment on `length` frames: length >= len(ref) + the pairs of equal neighbours."""
    ref = list(ref)
    return int(length) >= len(ref) + sum(1 for a, b in zip(ref[:-1], ref[1:]) if a == b)


def fit(x, utt_ptr, refs, n_phones, l2=1e-4, iters=200, gtol=1e-5, context=0, init=None):
    """A linear CTC model on the rows of x ((N, D) f32 on the device; utt_ptr (U + 1,); refs: one list of phone ids in
    [0, n_phones) per utterance), by probe.minimise on objective.  The blank is class n_phones.

    The rows are spliced with `context` frames per side first.  An utterance whose transcription has no alignment (too few
    frames) or more than 256 labels is dropped and counted before the first evaluation.  Standardisation as probe.fit: the
    float64 column mean and standard deviation of the rows used (a constant column gets std 1).  A phone that occurs in no
    transcription used keeps weights 0 and bias -inf.  init: None (zero parameters) or a frame-probe model of the same columns:
    its rows are copied, the blank row is zero, and its mean and std are taken over.  Same input: the same bits.

    -> (model: probe's keys with C = n_phones + 1 rows, plus "blank" and "context";
        history: probe.minimise's, plus "dropped_infeasible" and "utterances")"""
    import torch

    import phonerec
    import probe

    n_phones, context = int(n_phones), int(context)
    n_classes = n_phones + 1
    if n_phones < 1 or n_classes > CTC_MAX_CLASSES:
        raise ValueError("fit: %d phones, the CTC kernel takes 1 to %d (and the blank)" % (n_phones, CTC_MAX_CLASSES - 1))
    if iters < 0 or not l2 >= 0:
        raise ValueError("fit: iters = %r and l2 = %r must not be negative" % (iters, l2))
    x = _device("fit", "x", x, torch.float32, 2)
    utt = hip_ext.host_ptr("fit", "utt_ptr", utt_ptr)
    if utt[-1] != x.shape[0] or len(refs) != utt.shape[0] - 1:
        raise ValueError("fit: utt_ptr and refs do not describe the %d rows" % int(x.shape[0]))
    for r in refs:
        if len(r) and (min(r) < 0 or max(r) >= n_phones):
            raise ValueError("fit: a transcription holds a phone outside [0, %d)" % n_phones)
    lengths = np.diff(utt)
    keep = [u for u in range(len(refs)) if len(refs[u]) <= CTC_MAX_LABELS and feasible(lengths[u], refs[u])]
    dropped = len(refs) - len(keep)
    if not keep or int(lengths[keep].sum()) == 0:
        raise ValueError("fit: no utterance has an alignment")
    xs = splice(x, torch.from_numpy(utt).to(x.device), context)
    if dropped:
        rows = torch.from_numpy(probe.frames_of(keep, lengths)).to(x.device)
        xs = xs[rows].contiguous()
    D = int(xs.shape[1])
    if not bool(torch.isfinite(xs).all()):
        raise ValueError("fit: x holds values that are not finite")
    kept_refs = [refs[u] for u in keep]
    labels, lab_ptr = phonerec.csr(kept_refs, x.device)
    kept_ptr = np.concatenate([[0], np.cumsum(lengths[keep])]).astype(np.int64)
    prep = _Prepared("fit", xs, kept_ptr, labels, lab_ptr)
    params = np.zeros((n_classes, D + 1))
    if init is None:
        xd = xs.double()
        mu = xd.mean(dim=0)
        sd = ((xd - mu[None, :]) ** 2).mean(dim=0).sqrt()
        mean, std = mu.cpu().numpy(), sd.cpu().numpy()
        std = np.where(std > 0, std, 1.0)
    else:
        w, b, mean, std, _ = probe._model_arrays("fit", init)
        if w.shape != (n_phones, D):
            raise ValueError("fit: the initial model has weights %s, the data %d phones of %d columns" % (w.shape, n_phones, D))
        params[:n_phones, :D] = w
        params[:n_phones, D] = np.where(np.isfinite(b), b, 0.0)
    present = np.ones(n_classes, dtype=bool)
    present[:n_phones] = np.bincount(np.concatenate([np.asarray(r, dtype=np.int64) for r in kept_refs] + [np.zeros(0, np.int64)]),
                                     minlength=n_phones) > 0
    params[~present, :D] = 0.0
    params[~present, D] = -np.inf

    def fun(q):
        params[present] = q
        value, grad, _ = _objective_prepared(prep, params, n_phones, l2, mean, std)
        return value, grad[present]

    q, hist = probe.minimise(fun, params[present].copy(), iters, gtol)
    params[present] = q
    hist["dropped_infeasible"], hist["utterances"] = int(dropped), len(keep)
    model = {"weights": params[:, :D].copy(), "bias": params[:, D].copy(), "mean": np.asarray(mean, dtype=np.float64),
             "std": np.asarray(std, dtype=np.float64), "classes": np.arange(n_classes, dtype=np.float64),
             "blank": np.float64(n_phones), "context": np.float64(context)}
    return model, hist


# ------------------------------------------------------------------------------------------------------------------- decode
def greedy(x, utt_ptr, model, chunk=65536):
    """x (N, D) f32 and utt_ptr (U + 1,) int64 on one device, a model of fit() or load() -> (tokens int32, ptr int64 (U + 1,)):
    the rows spliced with the model's context, the arg-max class per row (the smallest index of equal logits), phonerec.collapse,
    then phonerec.fold with a table that maps the blank to -1.  Torch ops."""
    import torch

    import phonerec
    import probe

    w, b, mean, std, _ = probe._model_arrays("greedy", model)
    blank, context = int(model["blank"]), int(model["context"])
    ptr = torch.as_tensor(utt_ptr, dtype=torch.int64).to(x.device)
    xs = splice(x, ptr, context)
    if xs.shape[1] != w.shape[1]:
        raise ValueError("greedy: the spliced rows have %d columns, the model %d" % (xs.shape[1], w.shape[1]))
    tab, cst = probe.table(w, b, mean, std, device=x.device)
    wt = tab[:, :w.shape[1]].T.contiguous()
    pred = torch.empty(int(xs.shape[0]), dtype=torch.int32, device=x.device)
    for a in range(0, int(xs.shape[0]), int(chunk)):
        pred[a:a + chunk] = torch.argmax(xs[a:a + chunk] @ wt + cst[None, :], dim=1).to(torch.int32)
    table = np.arange(w.shape[0], dtype=np.int32)
    table[blank] = -1
    return phonerec.fold(*phonerec.collapse(pred, ptr), table)


def recognise(train_x, train_lengths, train_refs, test_x, test_lengths, test_refs, names, l2=1e-4, iters=200, gtol=1e-5, context=0,
              init=None, phone_table=None, model=None):
    """What both command lines do.  train_x, test_x (N, D) f32 on the device; the lengths are the frames per utterance; the refs
    one list of ids into `names` per utterance (no times).  Fit on the training transcriptions (or take `model`), decode the test
    utterances greedily, fold both sides through phone_table, phonerec.align, phonerec.error_rate.
    -> (model, report: error_rate's keys plus objective, iterations, converged, context, dropped_infeasible, l2; hyp, ref: the
    folded id lists per test utterance)"""
    import torch

    import phonerec

    n_phones = len(names)
    dev = test_x.device

    def ptr_of(lengths):
        return torch.from_numpy(np.concatenate([[0], np.cumsum(phonerec._host(lengths, np.int64))]).astype(np.int64)).to(dev)

    hist = {"iterations": 0, "converged": True, "objective": [float("nan")], "dropped_infeasible": 0}
    if model is None:
        model, hist = fit(train_x, ptr_of(train_lengths), train_refs, n_phones, l2=l2, iters=iters, gtol=gtol, context=context, init=init)
    test_ptr = ptr_of(test_lengths)
    if int(test_ptr[-1]) != int(test_x.shape[0]) or len(test_refs) != int(test_ptr.shape[0]) - 1:
        raise ValueError("test_lengths and test_refs do not describe the %d test rows" % int(test_x.shape[0]))
    table = np.arange(n_phones, dtype=np.int32) if phone_table is None else np.asarray(phone_table, dtype=np.int32)
    if table.shape != (n_phones,):
        raise ValueError("the phone table has %s entries for %d phones" % (table.shape, n_phones))
    hyp_tok, hyp_ptr = phonerec.fold(*greedy(test_x, test_ptr, model), table)
    ref_tok, ref_ptr = phonerec.fold(*phonerec.csr(test_refs, dev), table)
    report = phonerec.error_rate(phonerec.align(ref_tok, ref_ptr, hyp_tok, hyp_ptr))
    report.update({"objective": float(hist["objective"][-1]), "iterations": int(hist["iterations"]), "converged": bool(hist["converged"]),
                   "context": int(model["context"]), "dropped_infeasible": int(hist["dropped_infeasible"]), "l2": float(l2)})
    return model, report, phonerec.uncsr(hyp_tok, hyp_ptr), phonerec.uncsr(ref_tok, ref_ptr)


# --------------------------------------------------------------------------------------------------------------------- files
KEYS = ("weights", "bias", "mean", "std", "classes", "blank", "context")


def save(path, model):
    """One .npz with the probe's keys (C = n_phones + 1 rows) plus blank and context, float64."""
    import probe

    arrays = dict(zip(probe.KEYS, (np.ascontiguousarray(a) for a in probe._model_arrays("save", model))))
    arrays["blank"], arrays["context"] = np.float64(model["blank"]), np.float64(model["context"])
    with open(path, "wb") as fh:
        np.savez(fh, **arrays)


def load(path):
    """The inverse of save, its shapes checked."""
    import probe

    with np.load(path) as z:
        try:
            model = {key: np.asarray(z[key], dtype=np.float64) for key in KEYS}
        except KeyError as e:
            raise ValueError("%s holds no %s: not a file ctc.save wrote" % (path, e)) from None
    probe._model_arrays(path, model)
    if not 0 <= int(model["blank"]) < model["weights"].shape[0] or int(model["context"]) < 0:
        raise ValueError("%s: blank %s / context %s do not fit the %d classes" % (path, model["blank"], model["context"], model["weights"].shape[0]))
    return model
