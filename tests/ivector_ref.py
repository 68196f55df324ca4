"""A float64 numpy oracle of i-vector extraction (include/fhvae_ivector.h) that shares no code with ivector.py: dense inv / slogdet
per utterance, explicit loops over the components, its own posteriors and its own statistics.  A plain module, as tests/spk_ref.py."""
import numpy as np

SLICE = 1024
U24, U52 = 2.0 ** -24, 2.0 ** -52


def padded(D):
    return (D + 7) // 8 * 8


# ----------------------------------------------------------------------------------------------------------------- the UBM
def posteriors(x, ubm):
    """(N, D) rows -> (N, C) float64 posteriors of a diagonal-covariance mixture, by the log-sum-exp of the densities."""
    x = np.asarray(x, dtype=np.float64)
    w, mu, var = ubm["weights"], ubm["means"], ubm["variances"]
    ll = np.empty((x.shape[0], w.shape[0]))
    for c in range(w.shape[0]):
        d = x - mu[c]
        ll[:, c] = np.log(w[c]) - 0.5 * (np.log(2 * np.pi * var[c]).sum() + (d * d / var[c]).sum(axis=1))
    ll -= ll.max(axis=1, keepdims=True)
    p = np.exp(ll)
    return p / p.sum(axis=1, keepdims=True)


# -------------------------------------------------------------------------------------------------------------- statistics
def stats64(x32, post32, ptr):
    """The float64 sums of the f32 inputs -> (n (U, C), f (U, C, D), an (U, C) = sum g, af (U, C, D) = sum g |x|)."""
    x, g = np.asarray(x32, dtype=np.float64), np.asarray(post32, dtype=np.float64)
    U, C, D = len(ptr) - 1, g.shape[1], x.shape[1]
    n, f, af = np.zeros((U, C)), np.zeros((U, C, D)), np.zeros((U, C, D))
    for u in range(U):
        a, b = int(ptr[u]), int(ptr[u + 1])
        n[u] = g[a:b].sum(axis=0)
        f[u] = g[a:b].T @ x[a:b]
        af[u] = g[a:b].T @ np.abs(x[a:b])
    return n, f, n.copy(), af


def stats_bound(n, f, an, af):
    """The header's bound per entry: (SLICE + 3) 2^-24 sum g |a| + 2^-24 |total|."""
    return (SLICE + 3) * U24 * an + U24 * np.abs(n), (SLICE + 3) * U24 * af + U24 * np.abs(f)


def stats_sliced(x32, post32, ptr):
    """The kernel's slice definition on the same f32 inputs: per slice of SLICE rows from the utterance's first row one f32 chain
    over increasing rows, the slices added in float64 in order and rounded once -> (n, f) float32.  (The hardware adds four rows
    per instruction in its own order; this chain adds them one by one, so it agrees with the kernel within the bound, not bitwise.)"""
    x, g = np.asarray(x32, dtype=np.float32), np.asarray(post32, dtype=np.float32)
    U, C, D = len(ptr) - 1, g.shape[1], x.shape[1]
    n, f = np.zeros((U, C), np.float32), np.zeros((U, C, D), np.float32)
    for u in range(U):
        a, b = int(ptr[u]), int(ptr[u + 1])
        tn, tf = np.zeros(C), np.zeros((C, D))
        for s in range(a, b, SLICE):
            pn, pf = np.zeros(C, np.float32), np.zeros((C, D), np.float32)
            for t in range(s, min(b, s + SLICE)):
                pn = pn + g[t]
                pf = pf + g[t][:, None] * x[t][None, :]
            tn += pn
            tf += pf
        n[u], f[u] = tn, tf
    return n, f


def whiten(n, f, ubm):
    """(U, C), (U, C, D) -> ft (U, C, Dp) float64: (f_c - n_c m_c) / s_c, the padding columns 0."""
    U, C, D = f.shape
    ft = np.zeros((U, C, padded(D)))
    for c in range(C):
        ft[:, c, :D] = (f[:, c] - n[:, c, None] * ubm["means"][c]) / np.sqrt(ubm["variances"][c])
    return ft


# --------------------------------------------------------------------------------------------------------------- the model
def precision(nu, T):
    """L = I + sum_c n_c T_c^T T_c for one utterance; T (C, Dp, R)."""
    L = np.eye(T.shape[2])
    for c in range(T.shape[0]):
        L += nu[c] * (T[c].T @ T[c])
    return L


def refined_inverse(L):
    """inv(L) with one Newton step X + X (I - L X) in extended precision: the oracle's own error is far below the device's."""
    X = np.linalg.inv(L).astype(np.longdouble)
    Ll = L.astype(np.longdouble)
    X = X + X @ (np.eye(L.shape[0], dtype=np.longdouble) - Ll @ X)
    return X


def logdet(L):
    """log det of a symmetric positive definite L from the pivots of an elimination in extended precision."""
    A = np.array(L, dtype=np.longdouble)
    s = np.longdouble(0)
    for j in range(A.shape[0]):
        d = A[j, j]
        assert d > 0
        s += np.log(d)
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j] / d, A[j + 1:, j])
    return float(s)


def solve(L, b):
    """-> (w, E = L^-1 + w w^T, log det L) of one symmetric positive definite L, float64 (computed in extended precision)."""
    X = refined_inverse(L)
    w = X @ b.astype(np.longdouble)
    E = X + np.outer(w, w)
    return w.astype(np.float64), ((E + E.T) / 2).astype(np.float64), logdet(L)


def estep(n, ft, T):
    """n (U, C), ft (U, C, Dp), T (C, Dp, R) -> (w (U, R), E (U, R, R), Q)."""
    U, R = n.shape[0], T.shape[2]
    w, E, Q = np.zeros((U, R)), np.zeros((U, R, R)), 0.0
    for u in range(U):
        L = precision(n[u], T)
        b = np.zeros(R)
        for c in range(T.shape[0]):
            b += T[c].T @ ft[u, c]
        Li = np.linalg.inv(L)
        w[u] = Li @ b
        E[u] = Li + np.outer(w[u], w[u])
        Q += -0.5 * np.linalg.slogdet(L)[1] + 0.5 * b @ w[u]
    return w, E, Q


def objective(n, ft, T):
    return estep(n, ft, T)[2]


def mstep(n, ft, w, E):
    U, C, Dp = ft.shape
    R = w.shape[1]
    T = np.zeros((C, Dp, R))
    for c in range(C):
        A, K = np.zeros((R, R)), np.zeros((Dp, R))
        for u in range(U):
            A += n[u, c] * E[u]
            K += np.outer(ft[u, c], w[u])
        T[c] = K @ np.linalg.inv(A)
    return T


def start(C, D, R, seed):
    """0.1 times standard normal draws of default_rng(seed), shape (C, D, R), in (C, Dp, R) with zero padding rows."""
    T = np.zeros((C, padded(D), R))
    T[:, :D, :] = 0.1 * np.random.default_rng(seed).standard_normal((C, D, R))
    return T


def em(n, ft, T, iters, min_div=True):
    """-> ([T after every iteration], [Q after the start and after every step])."""
    Ts, Qs = [], []
    for _ in range(iters):
        w, E, Q = estep(n, ft, T)
        Qs.append(Q)
        T = mstep(n, ft, w, E)
        if min_div:
            w, E, Q = estep(n, ft, T)
            Qs.append(Q)
            G = np.linalg.cholesky(E.mean(axis=0))
            T = T @ G
        Ts.append(T)
    Qs.append(objective(n, ft, T))
    return Ts, Qs


# ----------------------------------------------------------------------------------------------------------------- figures
def cosine_eer(emb, labels):
    """The equal error rate of the cosine of all pairs i < j by sorting: the threshold where the miss and false-alarm rates cross
    (the mean of the two at the first threshold where FAR <= FRR)."""
    e = np.asarray(emb, dtype=np.float64)
    e = e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-300)
    i, j = np.triu_indices(e.shape[0], 1)
    s = (e[i] * e[j]).sum(axis=1)
    same = np.asarray(labels)[i] == np.asarray(labels)[j]
    order = np.argsort(s, kind="stable")
    same = same[order]
    frr = np.concatenate([[0], np.cumsum(same)]) / same.sum()          # targets rejected below the threshold
    far = 1.0 - np.concatenate([[0], np.cumsum(~same)]) / (~same).sum()  # non-targets accepted at or above it
    k = int(np.argmax(far <= frr))
    return float((far[k] + frr[k]) / 2)
