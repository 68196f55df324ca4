"""numpy oracle of exact t-SNE as csrc/tsne.hip defines it (the header of that file), taking a dtype:

  float64   the oracle: squared distances as sums of squared differences, everything in double
  float32   the model of what single precision costs: the expanded distance max(n_i + n_j - 2 x_i . x_j, 0) and every later
            operation in float32 (numpy's own summation orders, libm's exp): a kernel that is right differs from the oracle by
            about what this model differs from it

The tests allow the kernel FACTOR = 8 times the model's error (the MFMA chain's summation order, the device exp and the chunked
reduction differ from numpy's: first-order rounding effects of the model's own size), with a floor of FLOOR = 1e-6 under the
model's error ratios.
"""
import numpy as np

LO, HI, STEPS = -60.0, 60.0, 48  # bisection on log2 beta
FACTOR, FLOOR = 8.0, 1e-6


def make_case(N, D, clusters, seed):
    """Gaussian clusters, centres 2 randn and spread 0.7 -> (X (N, D) f32, label (N,)).  Every fifth seed has two exactly
    duplicated rows (m_i = 0 for both)."""
    rs = np.random.RandomState(seed)
    centre = 2.0 * rs.randn(clusters, D)
    label = rs.randint(0, clusters, size=N)
    X = (centre[label] + 0.7 * rs.randn(N, D)).astype(np.float32)
    if seed % 5 == 0:
        X[N // 2] = X[3]
        label[N // 2] = label[3]
    return X, label


def center(X):
    """Subtract the column means: computed in float64, rounded once (what tsne.py does on the way in)."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    return (X - X.mean(axis=0)).astype(np.float32)


def sqdist(X, dtype=np.float64):
    """(N, N) squared distances of f32 rows; the diagonal is 0."""
    X = np.asarray(X, dtype=np.float32).astype(dtype)
    N = X.shape[0]
    if dtype == np.float64:
        d2 = np.empty((N, N), dtype=np.float64)
        for r0 in range(0, N, 64):
            d = X[r0:r0 + 64, None, :] - X[None, :, :]
            d2[r0:r0 + 64] = (d * d).sum(axis=2)
    else:
        n = (X * X).sum(axis=1)
        d2 = np.maximum(n[:, None] + n[None, :] - dtype(2) * (X @ X.T), dtype(0))
    d2[np.arange(N), np.arange(N)] = 0
    return d2


def _row_sums(d2, beta, m):
    """-> e (zero diagonal), u = d2 - m (zero diagonal)"""
    N = d2.shape[0]
    u = d2 - m[:, None]
    u[np.arange(N), np.arange(N)] = 0
    e = np.exp(-(beta[:, None] * u))
    e[np.arange(N), np.arange(N)] = 0
    return e, u


def row_min(d2):
    N = d2.shape[0]
    return np.where(np.eye(N, dtype=bool), np.inf, d2).min(axis=1).astype(d2.dtype)


def entropy(d2, beta):
    """The entropy (nats) of every row's p_j|i at the given beta, in d2's dtype."""
    beta = np.asarray(beta).astype(d2.dtype)
    e, u = _row_sums(d2, beta, row_min(d2))
    s0 = e.sum(axis=1)
    return np.log(s0) + beta * (e * u).sum(axis=1) / s0


def affinity(d2, perplexity, lo=LO, hi=HI, steps=STEPS):
    """-> beta, m, Z in d2's dtype: the bisection of the kernel, no early exit."""
    dt = d2.dtype.type
    N = d2.shape[0]
    m = row_min(d2)
    lo, hi = np.full(N, lo, dtype=dt), np.full(N, hi, dtype=dt)
    target = dt(np.log(float(perplexity)))
    for _ in range(steps):
        mid = dt(0.5) * (lo + hi)
        beta = np.exp2(mid)
        e, u = _row_sums(d2, beta, m)
        s0 = e.sum(axis=1)
        up = np.log(s0) + beta * (e * u).sum(axis=1) / s0 > target
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    beta = np.exp2(dt(0.5) * (lo + hi))
    return beta, m, z_at(d2, beta, m)


def z_at(d2, beta, m=None):
    beta = np.asarray(beta).astype(d2.dtype)
    return _row_sums(d2, beta, row_min(d2) if m is None else m)[0].sum(axis=1)


def joint_p(d2, beta, m=None, Z=None):
    """p_ij = (p_j|i + p_i|j) / (2 N), zero diagonal, in d2's dtype."""
    dt = d2.dtype.type
    beta = np.asarray(beta).astype(d2.dtype)
    m = row_min(d2) if m is None else np.asarray(m).astype(d2.dtype)
    e, _ = _row_sums(d2, beta, m)
    Z = e.sum(axis=1) if Z is None else np.asarray(Z).astype(d2.dtype)
    c = e / Z[:, None]
    return (c + c.T) / dt(2 * d2.shape[0])


def gradient(P, Y, a=1.0):
    """-> dict F, R (N, 2), W (N,), Zq, grad (N, 2), kl, in P's dtype; differences first, as the kernel takes them."""
    dt = P.dtype.type
    Y = np.asarray(Y).astype(P.dtype)
    N = Y.shape[0]
    dy = Y[:, None, :] - Y[None, :, :]
    w = dt(1) / (dt(1) + (dy * dy).sum(axis=2))
    w[np.arange(N), np.arange(N)] = 0
    F = dt(a) * ((P * w)[:, :, None] * dy).sum(axis=1)
    R = ((w * w)[:, :, None] * dy).sum(axis=1)
    W = w.sum(axis=1)
    Zq = W.sum()
    ok = P > 0
    kl = (P[ok] * np.log(P[ok] * Zq / w[ok])).sum()
    return {"F": F, "R": R, "W": W, "Zq": Zq, "grad": dt(4) * (F - R / Zq), "kl": kl}


def fast_gradient(P, Y, a=1.0):
    """gradient()'s grad in float64 without (N, N, 2) arrays (for the long oracle runs; equal to 1e-12, test_tsne_cpu.py)."""
    Y = np.asarray(Y, dtype=np.float64)
    N = Y.shape[0]
    dy0, dy1 = Y[:, 0, None] - Y[None, :, 0], Y[:, 1, None] - Y[None, :, 1]
    w = 1.0 / (1.0 + dy0 * dy0 + dy1 * dy1)
    w[np.arange(N), np.arange(N)] = 0
    pw, ww = P * w, w * w
    F = a * np.stack([(pw * dy0).sum(axis=1), (pw * dy1).sum(axis=1)], axis=1)
    R = np.stack([(ww * dy0).sum(axis=1), (ww * dy1).sum(axis=1)], axis=1)
    return 4.0 * (F - R / w.sum())


def kl_divergence(P, Y):
    """float64 KL of the map Y against P."""
    return float(gradient(np.asarray(P, dtype=np.float64), np.asarray(Y, dtype=np.float64))["kl"])


def update(Y, V, G, grad, momentum, lr):
    """scikit-learn's _gradient_descent step -> Y, V, G (new arrays, the inputs' dtype)."""
    dt = Y.dtype.type
    inc = V * grad < 0
    G = np.where(inc, G + dt(0.2), G * dt(0.8))
    G = np.maximum(G, dt(0.01))
    V = dt(momentum) * V - dt(lr) * G * grad
    return Y + V, V, G


def schedule(it, exaggeration_iters=250):
    """-> (exaggeration, momentum) of iteration it (from 0)"""
    return (12.0, 0.5) if it < exaggeration_iters else (1.0, 0.8)


def learning_rate(N):
    return max(N / 48.0, 50.0)


def y0(N, seed):
    return (1e-4 * np.random.RandomState(seed).randn(N, 2)).astype(np.float32)


def run(P, Y, n_iter, lr, exaggeration_iters=250, V=None, G=None, start=0, fast=False):
    """n_iter iterations from Y (iteration numbers start .. start + n_iter - 1 of the schedule) -> Y, V, G in P's dtype."""
    Y = np.asarray(Y).astype(P.dtype)
    V = np.zeros_like(Y) if V is None else np.asarray(V).astype(P.dtype)
    G = np.ones_like(Y) if G is None else np.asarray(G).astype(P.dtype)
    for it in range(start, start + n_iter):
        a, mom = schedule(it, exaggeration_iters)
        grad = fast_gradient(P, Y, a) if fast else gradient(P, Y, a)["grad"]
        Y, V, G = update(Y, V, G, grad, mom, lr)
    return Y, V, G


def purity_1nn(Y, label):
    """The share of points whose nearest neighbour in the map has their label."""
    Y = np.asarray(Y, dtype=np.float64)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    d[np.arange(len(Y)), np.arange(len(Y))] = np.inf
    label = np.asarray(label)
    return float((label[d.argmin(axis=1)] == label).mean())


def ratio(got, ref):
    """The largest absolute error over the reference's largest magnitude."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def tolerance(model_ratio):
    return FACTOR * max(float(model_ratio), FLOOR)
