"""The oracle of gmm.py and csrc/gmm.hip, in numpy float64: the component log-densities from the SAME f32 table and constants the
device gets (so the table's own rounding cancels), the log-likelihood, the posteriors, the arg-max and its gap, the error bounds
of include/fhvae_gmm.h, the float64 statistics of any given posteriors, and an EM step (gmm.mstep's rules)."""
import math

import numpy as np

SLICE = 1024
U = 2.0 ** -24


def padded(width):
    return (int(width) + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------------------------- table
def table(weights, means, variances):
    """-> (tab (K, 2 Dp) f32, cst (K,) f32) of include/fhvae_gmm.h, from a float64 model, rounded once."""
    w, mu, var = (np.asarray(a, dtype=np.float64) for a in (weights, means, variances))
    K, D = mu.shape
    Dp = padded(D)
    tab = np.zeros((K, 2 * Dp), dtype=np.float64)
    tab[:, :D] = mu / var
    tab[:, Dp:Dp + D] = -1.0 / (2.0 * var)
    with np.errstate(divide="ignore"):
        cst = np.log(w) - (D * math.log(2.0 * math.pi) + np.log(var).sum(axis=1) + (mu * mu / var).sum(axis=1)) / 2.0
    return tab.astype(np.float32), cst.astype(np.float32)


def pad_rows(x):
    x = np.asarray(x, dtype=np.float32)
    return np.pad(x, ((0, 0), (0, padded(x.shape[1]) - x.shape[1])))


# ------------------------------------------------------------------------------------------------------------------ E-step
def scores(x, tab, cst):
    """x (N, D) f32, the device's f32 tab and cst -> (l (N, K) float64, M (N, K): |cst[k]| + sum_d (|x p1| + x^2 |p2|), the
    magnitudes the f32 chain's error is bounded by)."""
    x = pad_rows(x).astype(np.float64)
    tab, cst = np.asarray(tab, dtype=np.float64), np.asarray(cst, dtype=np.float64)
    Dp = x.shape[1]
    assert tab.shape[1] == 2 * Dp and cst.shape[0] == tab.shape[0]
    feat = np.concatenate([x, x * x], axis=1)
    l = feat @ tab.T + cst[None, :]
    acst = np.where(np.isfinite(cst), np.abs(cst), 0.0)  # (a weight-0 component: l = -inf exactly, no error to bound)
    M = np.abs(feat) @ np.abs(tab).T + acst[None, :]
    return l, M


def estep(x, tab, cst):
    """-> dict: l, loglik (N,), post (N, K), labels (the first of equal float64 values), gap (best minus runner-up; inf when
    K = 1), E (N, K) = (2 Dp + 2) u M, Emax (N,), B_ll (N,), B_post (N,): the relative bound of a posterior."""
    l, M = scores(x, tab, cst)
    N, K = l.shape
    Dp = tab.shape[1] // 2
    m = l.max(axis=1)
    s = np.exp(l - m[:, None]).sum(axis=1)
    loglik = m + np.log(s)
    post = np.exp(l - loglik[:, None])
    labels = l.argmax(axis=1)
    gap = m - np.partition(l, K - 2, axis=1)[:, K - 2] if K > 1 else np.full(N, np.inf)
    E = (2 * Dp + 2) * U * M
    Emax = E.max(axis=1)
    return {"l": l, "loglik": loglik, "post": post, "labels": labels.astype(np.int32), "gap": gap, "E": E, "Emax": Emax,
            "B_ll": Emax + (K + 8) * U + 2 * U * np.abs(loglik), "B_post": 2 * Emax + (K + 16) * U}


def direct_loglik(x, weights, means, variances):
    """log sum_k w_k N(x; mu_k, diag var_k) in float64, straight from the density (weight-0 components skipped)."""
    x, w, mu, var = (np.asarray(a, dtype=np.float64) for a in (x, weights, means, variances))
    out = np.zeros(x.shape[0])
    for n in range(x.shape[0]):
        terms = [math.log(w[k]) - 0.5 * float(np.sum(np.log(2.0 * math.pi * var[k]) + (x[n] - mu[k]) ** 2 / var[k]))
                 for k in range(w.shape[0]) if w[k] > 0]
        top = max(terms)
        out[n] = top + math.log(sum(math.exp(t - top) for t in terms))
    return out


# -------------------------------------------------------------------------------------------------------------- statistics
def stats(x, post):
    """The float64 sums of ANY given post (the device's own, in the tests) -> (nk (K,), sx (K, D), sxx (K, D), and the bounds'
    magnitudes: sum_n post, sum_n post |x|, sum_n post x^2)."""
    x, post = np.asarray(x, dtype=np.float64), np.asarray(post, dtype=np.float64)
    nk = post.sum(axis=0)
    sx, sxx = post.T @ x, post.T @ (x * x)
    return nk, sx, sxx, (np.abs(post).sum(axis=0), np.abs(post).T @ np.abs(x), np.abs(post).T @ (x * x))


def stats_bound(mag):
    return (SLICE + 3) * U * mag


# ------------------------------------------------------------------------------------------------------------------ M-step
def mstep(nk, sx, sxx, prev_means, prev_variances, n, global_var, var_floor=0.01, min_count=3.0):
    """-> (weights, means, variances, starved, floored), component by component."""
    nk, sx, sxx = (np.asarray(a, dtype=np.float64) for a in (nk, sx, sxx))
    K, D = sx.shape
    w, mu, var = nk / float(n), np.array(prev_means, dtype=np.float64), np.array(prev_variances, dtype=np.float64)
    starved = floored = 0
    for k in range(K):
        if nk[k] < min_count:
            starved += 1
            continue
        for d in range(D):
            mu[k, d] = sx[k, d] / nk[k]
            v = sxx[k, d] / nk[k] - mu[k, d] * mu[k, d]
            f = var_floor * float(global_var[d])
            if v < f:
                floored += 1
                v = f
            var[k, d] = v
    return w, mu, var, starved, floored


def em_step(x, weights, means, variances, global_var, var_floor=0.01, min_count=3.0):
    """One EM iteration in float64 (from the f32 table, as the device) -> (mean loglik of the model given, the new model)."""
    tab, cst = table(weights, means, variances)
    e = estep(x, tab, cst)
    nk, sx, sxx, _ = stats(x, e["post"])
    new = mstep(nk, sx, sxx, means, variances, np.asarray(x).shape[0], global_var, var_floor, min_count)
    return float(e["loglik"].mean()), new[:3]


# ------------------------------------------------------------------------------------------------------------------ inputs
def case(N, K, D, seed=0):
    """The inputs of the GPU tests: x, mu ~ N(0, 1), var = exp(U(-1, 1)), Dirichlet(5) weights, seeded from (N, K, D)."""
    rng = np.random.default_rng(1000003 * N + 1009 * K + D + 7919 * seed)
    x = rng.standard_normal((N, D)).astype(np.float32)
    mu = rng.standard_normal((K, D))
    var = np.exp(rng.uniform(-1.0, 1.0, (K, D)))
    w = rng.dirichlet(np.full(K, 5.0))
    return x, w, mu, var
