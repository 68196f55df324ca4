"""float64 numpy oracle of the speaker back end (csrc/spk.hip, spk_backend.py); it shares no code with spk_backend.py.

The model: planted two-covariance data, a fit written straight from the formulas (explicit inverses, a loop over the classes),
the LLR as a log-density ratio of dense 2K-dimensional Gaussians, the dense marginal log-likelihood of a class.

The kernels: the f32 tables are promoted to float64 and everything is computed there.
  project   y_k = sum_d A_kd (x_d - m_d) with the difference rounded to f32 as the kernel rounds it; the kernel's chain of Din
            fmaf is within (Din + 2) 2^-24 sum_d |A_kd| |x_d - m_d| of it
  score     s_ij = v_i . v_j + a_i + a_j + c.  The kernel's f32 score and its bin can differ from the float64 ones by
                delta_ij = 2^-24 [(Dp + 3) M_ij + 4 (hi - lo)],   M_ij = sum_k |v_ik v_jk| + |a_i| + |a_j| + |c|
            Dp fma roundings of the dot (Dp the padded width), two additions (one more rounding of a_i + a_j counted with
            them), and the four roundings of the bin arithmetic (s - lo, hi - lo, NB / (hi - lo), the product), each at most
            2^-24 (hi - lo) on the score axis.  So for every edge the kernel's count of trials in bins >= k differs from the
            oracle's by at most the number of trials within their delta of that edge.
"""
import numpy as np

U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ the data
def planted(seed, speakers, rows, K, nuisance=6.0, between=1.0, spread=0.3):
    """Two-covariance data: speaker offsets ~ N(0, between^2 diag(g)), g from 1 down to 0.2, noise ~ N(0, W) with W = 0.6^2 I
    plus one strong direction (nuisance^2 n n^T, n random) that a raw cosine cannot ignore; `rows` per speaker on average
    (1 + Poisson unless spread == 0) -> (x (N, K) f32, label (N,) int32)."""
    rs = np.random.RandomState(seed)
    g = np.linspace(1.0, 0.2, K)
    n = np.random.RandomState(4242 + K).randn(K)  # (the model's, not the draw's: training and held-out sets share it)
    n /= np.linalg.norm(n)
    counts = np.full(speakers, rows) if spread == 0 else np.maximum(1, rs.poisson(rows, size=speakers))
    label = np.repeat(np.arange(speakers), counts).astype(np.int32)
    centre = 3.0 + between * rs.randn(speakers, K) * g
    x = centre[label] + 0.6 * rs.randn(len(label), K) + nuisance * rs.randn(len(label), 1) * n
    perm = rs.permutation(len(label))
    return x[perm].astype(np.float32), label[perm]


# ------------------------------------------------------------------------------------------------------------------ the model
def class_stats(x, label):
    keep = label >= 0
    x, label = np.asarray(x, dtype=np.float64)[keep], label[keep]
    names = np.unique(label)
    m = x.mean(axis=0)
    K = x.shape[1]
    Sw, Sb, means, counts = np.zeros((K, K)), np.zeros((K, K)), [], []
    for s in names:
        xc = x[label == s]
        mc = xc.mean(axis=0)
        Sw += (xc - mc).T @ (xc - mc)
        Sb += len(xc) * np.outer(mc - m, mc - m)
        means.append(mc)
        counts.append(len(xc))
    return x, m, np.asarray(means), np.asarray(counts), Sw, Sb


def diagonalise(within, between, top=None):
    L = np.linalg.cholesky(within)
    Li = np.linalg.inv(L)
    e, Uv = np.linalg.eigh(Li @ between @ Li.T)
    order = np.argsort(-e)[:top]
    return Uv[:, order].T @ Li, e[order]


def em_step(B, W, Sw, d, counts):
    """The issue's formulas as written: P_c = B^-1 + n_c W^-1, yhat_c = P_c^-1 n_c W^-1 d_c."""
    Bi, Wi = np.linalg.inv(B), np.linalg.inv(W)
    Bn, Wn = np.zeros_like(B), Sw.copy()
    for dc, n in zip(d, counts):
        Pinv = np.linalg.inv(Bi + n * Wi)
        yh = Pinv @ (n * Wi @ dc)
        Bn += Pinv + np.outer(yh, yh)
        Wn += n * (Pinv + np.outer(dc - yh, dc - yh))
    return Bn / len(counts), Wn / counts.sum()


def fit(x, label, lda_dim=None, length_norm=True, iters=10, ridge=1e-8):
    """-> dict: m, A_lda (or None), length_norm, m2, W, B, A_p, psi, and Sw_lda (the ridged within-class scatter / N of the LDA)."""
    x, m, _, counts, Sw, Sb = class_stats(x, label)
    lab = label[label >= 0]
    N, D = x.shape
    A_lda, Sw_lda = None, None
    y = x - m
    if lda_dim is not None:
        Sw_lda = (Sw + ridge * np.trace(Sw) / D * np.eye(D)) / N
        A_lda, _ = diagonalise(Sw_lda, Sb / N, lda_dim)
        y = y @ A_lda.T
    K = y.shape[1]
    if length_norm:
        y = y * (np.sqrt(K) / np.maximum(np.sqrt((y * y).sum(axis=1)), 1e-30))[:, None]
    y, m2, means, counts, Sw2, Sb2 = class_stats(y, lab)
    W = Sw2 / N
    W = W + ridge * np.trace(W) / K * np.eye(K)
    B = Sb2 / len(counts)
    for _ in range(iters):
        B, W = em_step(B, W, Sw2, means - m2, counts)
    A_p, psi = diagonalise(W, B)
    return {"m": m, "A_lda": A_lda, "length_norm": length_norm, "m2": m2, "W": W, "B": B, "A_p": A_p, "psi": np.maximum(psi, 0.0),
            "Sw_lda": Sw_lda}


def terms(psi):
    p = psi / (2 * psi + 1)
    q = psi ** 2 / (2 * (psi + 1) * (2 * psi + 1))
    return p, q, 0.5 * np.sum(2 * np.log(1 + psi) - np.log(1 + 2 * psi))


def tables(model):
    """The f32 tables the kernels read, from a fit() dict: A1, m, A_p, m2, q, sqrt_p (float32 arrays) and c (a float32 value)."""
    p, q, c = terms(model["psi"])
    A1 = np.eye(len(model["m"])) if model["A_lda"] is None else model["A_lda"]
    f = lambda t: np.ascontiguousarray(t, dtype=np.float32)  # noqa: E731
    return {"A1": f(A1), "m": f(model["m"]), "A_p": f(model["A_p"]), "m2": f(model["m2"]), "q": f(q), "sqrt_p": f(np.sqrt(p)),
            "c": float(np.float32(c))}


def transform64(model, x):
    """x (S, D) -> u (S, K) float64 by the float64 model (no f32 anywhere)."""
    y = np.asarray(x, dtype=np.float64) - model["m"]
    if model["A_lda"] is not None:
        y = y @ model["A_lda"].T
    if model["length_norm"]:
        y = y * (np.sqrt(y.shape[1]) / np.maximum(np.sqrt((y * y).sum(axis=1)), 1e-30))[:, None]
    return y, (y - model["m2"]) @ model["A_p"].T


def llr_closed(model, u):
    """(S, S) closed-form LLR of rows u."""
    p, q, c = terms(model["psi"])
    a = -(q * u * u).sum(axis=1)
    return (u * p) @ u.T + a[:, None] + a[None, :] + c


def log_gauss(x, cov):
    sign, logdet = np.linalg.slogdet(cov)
    assert sign > 0
    return -0.5 * (len(x) * np.log(2 * np.pi) + logdet + x @ np.linalg.solve(cov, x))


def llr_dense(yi, yj, m2, B, W):
    """log N([yi; yj]; same speaker) - log N(yi) - log N(yj): dense 2K-dimensional Gaussians."""
    T = B + W
    joint = np.block([[T, B], [B, T]])
    return log_gauss(np.concatenate([yi - m2, yj - m2]), joint) - log_gauss(yi - m2, T) - log_gauss(yj - m2, T)


def class_loglik(yc, m2, B, W):
    """log N(vec(yc - m2); 0, I (x) W + 1 1^T (x) B) of one class's rows (n, K), dense."""
    n, K = yc.shape
    cov = np.kron(np.eye(n), W) + np.kron(np.ones((n, n)), B)
    return log_gauss((yc - m2).reshape(-1), cov)


# ---------------------------------------------------------------------------------------------------------------- the kernels
def project(x, A, mean, normalise=False, q=None, scale=None):
    """-> (out (S, K) float64, a (S,) float64 or None, y (S, K) the unnormalised products, bound (S, K) = sum_d |A_kd| |x_d - m_d|)."""
    t = (np.asarray(x, dtype=np.float32) - np.asarray(mean, dtype=np.float32)).astype(np.float64)  # (the kernel's one rounding)
    A = np.asarray(A, dtype=np.float64)
    y0 = t @ A.T
    bound = np.abs(t) @ np.abs(A).T
    y = y0
    if normalise:
        y = y * (np.sqrt(A.shape[0]) / np.maximum(np.sqrt((y * y).sum(axis=1)), 1e-30))[:, None]
    a = None if q is None else -(np.asarray(q, dtype=np.float64) * y * y).sum(axis=1)
    out = y if scale is None else y * np.asarray(scale, dtype=np.float64)
    return out, a, y0, bound


def transform32(tab, x, length_norm):
    """The two stages on the f32 tables with every stage's result rounded to f32, as the device holds it -> (v (S, Dp) f32
    zero-padded to a multiple of 16, a (S,) f32)."""
    y = project(x, tab["A1"], tab["m"], normalise=length_norm)[0].astype(np.float32)
    v, a, _, _ = project(y, tab["A_p"], tab["m2"], q=tab["q"], scale=tab["sqrt_p"])
    K = v.shape[1]
    vp = np.zeros((v.shape[0], (K + 15) // 16 * 16), dtype=np.float32)
    vp[:, :K] = v
    return vp, a.astype(np.float32)


def trials(label):
    """-> (i, j, same) of the trials i < j with both labels >= 0."""
    label = np.asarray(label)
    i, j = np.triu_indices(len(label), k=1)
    ok = (label[i] >= 0) & (label[j] >= 0)
    i, j = i[ok], j[ok]
    return i, j, label[i] == label[j]


def scores(v, a, c, i, j):
    """float64 s and M of the pairs (i, j) on the f32 tables."""
    v, a = np.asarray(v, dtype=np.float64), np.asarray(a, dtype=np.float64)
    dot = np.einsum("nk,nk->n", v[i], v[j])
    M = np.einsum("nk,nk->n", np.abs(v[i]), np.abs(v[j])) + np.abs(a[i]) + np.abs(a[j]) + abs(float(c))
    return dot + a[i] + a[j] + float(c), M


def delta(M, Dp, lo=0.0, hi=0.0):
    return U * ((Dp + 3) * M + 4.0 * (float(hi) - float(lo)))


def edge_counts(s, dlt, lo, hi, NB):
    """For every edge k in 0..NB (edge k at lo + k (hi - lo) / NB): (trials in bins >= k, trials within their own dlt of edge k,
    the histogram).  The clamp puts every trial in a bin >= 0 and none in a bin >= NB: the outer edges are exact.  hi == lo:
    every trial is in bin 0."""
    s, dlt = np.asarray(s, dtype=np.float64), np.asarray(dlt, dtype=np.float64)
    lo, hi = float(lo), float(hi)
    if hi == lo:
        hist = np.zeros(NB, dtype=np.int64)
        hist[0] = len(s)
        cum = np.zeros(NB + 1, dtype=np.int64)
        cum[0] = len(s)
        return cum, np.zeros(NB + 1, dtype=np.int64), hist
    w = (hi - lo) / NB
    bins = np.clip(np.floor((s - lo) / w), 0, NB - 1).astype(np.int64)
    hist = np.bincount(bins, minlength=NB)
    cum = np.concatenate([np.cumsum(hist[::-1])[::-1], [0]])
    first = np.ceil((s - dlt - lo) / w).astype(np.int64)   # the edges k with |s - edge_k| <= dlt are first .. last
    last = np.floor((s + dlt - lo) / w).astype(np.int64)
    has = (last >= first) & (last >= 1) & (first <= NB - 1)
    first, last = np.clip(first[has], 1, NB - 1), np.clip(last[has], 1, NB - 1)
    diff = np.zeros(NB + 2, dtype=np.int64)
    np.add.at(diff, first, 1)
    np.add.at(diff, last + 1, -1)
    near = np.cumsum(diff)[:NB + 1]
    near[0] = near[NB] = 0
    return cum, near, hist


def exact_eer(tar, non):
    """The EER from the sorted float64 scores: thresholds at every distinct score (accept iff score >= threshold) and above
    the largest; where |FRR - FAR| is smallest, their mean."""
    tar, non = np.sort(tar), np.sort(non)
    th = np.unique(np.concatenate([tar, non]))
    frr = np.concatenate([np.searchsorted(tar, th, side="left"), [len(tar)]]) / len(tar)
    far = np.concatenate([len(non) - np.searchsorted(non, th, side="left"), [0]]) / len(non)
    k = int(np.argmin(np.abs(frr - far)))
    return 0.5 * (frr[k] + far[k])


def cosine_scores(x, i, j):
    x = np.asarray(x, dtype=np.float64)
    n = np.maximum(np.sqrt((x * x).sum(axis=1)), 1e-30)
    return np.einsum("nk,nk->n", x[i], x[j]) / (n[i] * n[j])
