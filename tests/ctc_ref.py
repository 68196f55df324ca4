"""A float64 numpy oracle of include/fhvae_ctc.h, written from the header and not from the kernel: the log-domain forward-backward
pass of one utterance, vectorised over the trellis states per frame (T = 3000 takes well under a second), and the host side of
ctc.objective.

  log_softmax  lp_t[c] = (z - m) - log sum exp(z - m)
  loss         one utterance -> (nll, grad (T, C) float64 or None, flag)
  batch        a CSR batch -> (nll (U,), grad (N, C) float64, status)
  brute_force  -log of the summed probability of every alignment that collapses to the labels (T <= 5 or so)
  objective    the value and the gradient of ctc.objective from given f32 logits, in float64
  collapse     the greedy decode of an arg-max sequence
"""
import itertools

import numpy as np

BAD_LABEL, INFEASIBLE = 2, 4
MAX_LABELS = 256
NEG = -np.inf


def lse(*xs):
    """m + log(sum exp(x - m)) elementwise over the arrays given, m the largest; -inf where every x is -inf."""
    xs = np.stack([np.asarray(x, dtype=np.float64) for x in xs])
    m = xs.max(axis=0)
    mm = np.where(np.isneginf(m), 0.0, m)
    with np.errstate(divide="ignore"):
        return mm + np.log(np.exp(xs - mm).sum(axis=0))


def log_softmax(z):
    z = np.asarray(z, dtype=np.float64)
    d = z - z.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        return d - np.log(np.exp(d).sum(axis=1, keepdims=True))


def loss(z, labels, blank, want_grad=True):
    """z (T, C) f32 or float64 logits, labels a sequence of ints -> (nll, grad (T, C) float64 (None if not wanted), flag)."""
    z = np.asarray(z)
    T, C = z.shape
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    L = labels.shape[0]
    zero = np.zeros((T, C)) if want_grad else None
    if L > MAX_LABELS or (L and (labels.min() < 0 or labels.max() >= C or (labels == blank).any())):
        return np.inf, zero, BAD_LABEL
    if T == 0:
        return (0.0, zero, 0) if L == 0 else (np.inf, zero, INFEASIBLE)
    S = 2 * L + 1
    ext = np.full(S, blank, dtype=np.int64)
    ext[1::2] = labels
    skip = np.zeros(S, dtype=bool)
    skip[3::2] = labels[1:] != labels[:-1]
    with np.errstate(invalid="ignore", over="ignore"):
        lp = log_softmax(z)
        le = lp[:, ext]  # (T, S): lp_t[l'_s]
        alpha = np.full((T, S), NEG)
        alpha[0, 0] = le[0, 0]
        if S > 1:
            alpha[0, 1] = le[0, 1]
        pad1, pad2 = np.full(1, NEG), np.full(2, NEG)
        for t in range(1, T):
            p = alpha[t - 1]
            p1 = np.concatenate([pad1, p[:-1]])
            p2 = np.where(skip, np.concatenate([pad2, p[:-2]])[:S], NEG)
            alpha[t] = lse(p, p1, p2) + le[t]
        ll = float(lse(alpha[T - 1, S - 1], alpha[T - 1, S - 2] if S > 1 else NEG))
        if np.isneginf(ll):
            return np.inf, zero, INFEASIBLE
        if not want_grad:
            return -ll, None, 0
        beta = np.full((T, S), NEG)
        beta[T - 1, max(S - 2, 0):] = 0.0
        for t in range(T - 2, -1, -1):
            g = beta[t + 1] + le[t + 1]
            n1 = np.concatenate([g[1:], pad1])
            n2 = np.concatenate([np.where(skip, g, NEG)[2:], pad2])[:S]
            beta[t] = lse(g, n1, n2)
        post = np.exp(alpha + beta - ll)
        grad = np.exp(lp)
        for t in range(T):
            grad[t] -= np.bincount(ext, weights=post[t], minlength=C)  # (summed in increasing s)
    return -ll, grad, 0


def batch(z, utt_ptr, labels, lab_ptr, blank, want_grad=True):
    """-> (nll (U,) float64, grad (N, C) float64 or None, status)."""
    z = np.asarray(z)
    U = len(utt_ptr) - 1
    nll = np.zeros(U)
    grad = np.zeros(z.shape, dtype=np.float64) if want_grad else None
    status = 0
    for u in range(U):
        a, b = int(utt_ptr[u]), int(utt_ptr[u + 1])
        nll[u], g, flag = loss(z[a:b], labels[int(lab_ptr[u]):int(lab_ptr[u + 1])], blank, want_grad)
        status |= flag
        if want_grad:
            grad[a:b] = g
    return nll, grad, status


def collapse(path, blank):
    """Runs merged, then the blank dropped."""
    out, last = [], None
    for v in path:
        if v != last and v != blank:
            out.append(int(v))
        last = v
    return out


def brute_force(z, labels, blank):
    """-log of the sum over all C^T paths that collapse to `labels` of the product of the softmax probabilities."""
    z = np.asarray(z, dtype=np.float64)
    T, C = z.shape
    p = np.exp(log_softmax(z)) if T else np.zeros((0, C))
    total = 0.0
    want = [int(v) for v in labels]
    for path in itertools.product(range(C), repeat=T):
        if collapse(path, blank) == want:
            total += float(np.prod([p[t, c] for t, c in enumerate(path)]))
    with np.errstate(divide="ignore"):
        return -np.log(total)


def feasible(T, labels):
    labels = list(labels)
    return T >= len(labels) + sum(1 for a, b in zip(labels[:-1], labels[1:]) if a == b)


def objective(logits, x, utt_ptr, labels, lab_ptr, blank, params, l2, mean, std):
    """The host side of ctc.objective in float64 from given logits (N, C) and raw rows x (N, D): value = sum nll / N + l2 / 2
    ||w||^2; the gradient by the chain rule through z = (x - mean) / std, from the unrounded float64 r.
    -> (value, grad (C, D + 1), nll (U,), r (N, C))"""
    x = np.asarray(x, dtype=np.float64)
    N, D = x.shape
    nll, r, _ = batch(logits, utt_ptr, labels, lab_ptr, blank)
    w = params[:, :D]
    value = nll.sum() / N + 0.5 * l2 * float(np.sum(w * w))
    zs = (x - mean[None, :]) / std[None, :]
    grad = np.empty_like(params)
    grad[:, :D] = r.T @ zs / N + l2 * w
    grad[:, D] = r.sum(axis=0) / N
    return float(value), grad, nll, r
