"""The oracle of probe.py and csrc/probe.hip, in numpy float64: the logits from the SAME f32 table and bias the device gets (so the
table's own rounding cancels), the log-sum-exp, the arg-max and its runner-up gap, the negative log-likelihood, the totals, the
gradient, the objective with its chain rule through the standardisation, and the error bounds of include/fhvae_probe.h.

THE BOUNDS, derived (u = 2^-24, the unit roundoff of f32; W the padded width; C the classes):
  M(n, c) = |cst[c]| + sum_d |x[n][d]| |tab[c][d]|
  E(n, c) = (W + 2) u M(n, c)          a logit: W fused steps of the chain and the addition of cst are W + 1 roundings, each at
                                       most u times a partial sum that M bounds; one more u M of slack
  Emax(n) = max_c E(n, c)
  B_lse(n) = Emax(n) + (C + 8) u + 2 u |lse[n]|
                                       the form of B_ll in DESIGN section 25: shifting every logit by at most Emax shifts the
                                       log-sum-exp by at most Emax; C additions and C expf of a few ulp each change log s by at
                                       most (C + 8) u; logf and the last addition are relative to |lse|
  B_nll(n) = B_lse(n) + E(n, y[n])     lse - l(n, y): the two errors add (the rounding of the difference, u |nll| <=
                                       u (|lse| + |l|), lies within the slack of the two terms)
  B_post(n) = 2 Emax(n) + (C + 16) u   the relative bound of a posterior p = expf(l - lse), as in section 25
  B_grad[c][d] = sum_n (B_post(n) p(n, c) + 2^-126) |x[n][d]|  +  (SLICE + 3) u sum_n |r(n, c)| |x[n][d]|
                                       over the labelled rows; |x| is 1 for the bias column.  The first term is the error of
                                       the residual r = p - onehot that enters the sum, the second the f32 chain of a slice
                                       (SLICE roundings at most, each relative to a partial sum that sum |r| |x| bounds; the
                                       rounding of the subtraction p - onehot, u |r|, lies within the + 3) and the float64
                                       sum over the slices, which is far below either.
"""
import numpy as np

SLICE = 1024
U = 2.0 ** -24


def padded(width):
    return (int(width) + 15) // 16 * 16


def pad_rows(x):
    x = np.asarray(x)
    return np.pad(x, ((0, 0), (0, padded(x.shape[1]) - x.shape[1])))


def table(weights, bias, mean=None, std=None, f32=True):
    """-> (tab (C, W), cst (C,)) of include/fhvae_probe.h from a float64 model, rounded once to f32 (f32=False: left in float64)."""
    w, b = np.asarray(weights, dtype=np.float64), np.asarray(bias, dtype=np.float64)
    D = w.shape[1]
    mean = np.zeros(D) if mean is None else np.asarray(mean, dtype=np.float64)
    std = np.ones(D) if std is None else np.asarray(std, dtype=np.float64)
    tab = np.zeros((w.shape[0], padded(D)))
    tab[:, :D] = w / std[None, :]
    cst = b - (tab[:, :D] * mean[None, :]).sum(axis=1)
    return (tab.astype(np.float32), cst.astype(np.float32)) if f32 else (tab, cst)


def logits(x, tab, cst):
    """-> (l (N, C) float64, M (N, C))"""
    x = pad_rows(x).astype(np.float64)
    tab, cst = np.asarray(tab, dtype=np.float64), np.asarray(cst, dtype=np.float64)
    assert tab.shape[1] == x.shape[1] and cst.shape == (tab.shape[0],)
    return x @ tab.T + cst[None, :], np.abs(x) @ np.abs(tab).T + np.abs(cst)[None, :]


def forward(x, y, tab, cst):
    """-> dict: l, lse (N,), p (N, C), pred (the first of equal float64 values), gap (best minus runner-up; inf when C = 1), nll
    (0 for an unlabelled row), labelled (bool), totals (sum nll, labelled, correct), E, Emax, B_lse, B_nll, B_post."""
    l, M = logits(x, tab, cst)
    N, C = l.shape
    y = np.asarray(y).astype(np.int64)
    lab = (y >= 0) & (y < C)
    W = np.asarray(tab).shape[1]
    m = l.max(axis=1)
    lse = m + np.log(np.exp(l - m[:, None]).sum(axis=1))
    p = np.exp(l - lse[:, None])
    pred = l.argmax(axis=1).astype(np.int32)
    gap = m - np.partition(l, C - 2, axis=1)[:, C - 2] if C > 1 else np.full(N, np.inf)
    ys = np.where(lab, y, 0)
    rows = np.arange(N)
    nll = np.where(lab, lse - l[rows, ys], 0.0)
    E = (W + 2) * U * M
    Emax = E.max(axis=1)
    B_lse = Emax + (C + 8) * U + 2 * U * np.abs(lse)
    totals = np.array([nll.sum(), float(lab.sum()), float((lab & (pred == y)).sum())])
    return {"l": l, "lse": lse, "p": p, "pred": pred, "gap": gap, "nll": nll, "labelled": lab, "totals": totals, "E": E, "Emax": Emax,
            "B_lse": B_lse, "B_nll": np.where(lab, B_lse + E[rows, ys], 0.0), "B_post": 2 * Emax + (C + 16) * U}


def residuals(f, y):
    """r (N, C) = p - onehot on the labelled rows, 0 on the others"""
    y = np.asarray(y).astype(np.int64)
    r = f["p"].copy()
    lab = f["labelled"]
    r[np.nonzero(lab)[0], y[lab]] -= 1.0
    r[~lab] = 0.0
    return r


def grad(x, y, tab, cst, f=None):
    """-> (grad (C, W + 1) float64: sum_n r(n, c) [x[n], 1], the bias column last; B_grad of the same shape)"""
    f = forward(x, y, tab, cst) if f is None else f
    r = residuals(f, y)
    lab = f["labelled"].astype(np.float64)
    x1 = np.concatenate([pad_rows(x).astype(np.float64), np.ones((r.shape[0], 1))], axis=1)
    dr = (f["B_post"][:, None] * f["p"] + 2.0 ** -126) * lab[:, None]
    return r.T @ x1, dr.T @ np.abs(x1) + (SLICE + 3) * U * (np.abs(r).T @ np.abs(x1))


def objective(params, x, y, l2, mean=None, std=None, f32=False, with_bound=False):
    """The objective of probe.objective in float64: params (C, D + 1) in the standardised coordinates -> (value, gradient).
    f32=True: through the f32 table, as the device; with_bound: also B_grad carried through the same chain rule."""
    params = np.asarray(params, dtype=np.float64)
    D = params.shape[1] - 1
    mean = np.zeros(D) if mean is None else np.asarray(mean, dtype=np.float64)
    std = np.ones(D) if std is None else np.asarray(std, dtype=np.float64)
    tab, cst = table(params[:, :D], params[:, D], mean, std, f32=f32)
    f = forward(x, y, tab, cst)
    n = f["totals"][1]
    if n == 0:
        out = (0.0, np.zeros_like(params))
        return out + (np.zeros_like(params),) if with_bound else out
    G, B = grad(x, y, tab, cst, f)
    W = tab.shape[1]
    w = params[:, :D]
    g = np.empty_like(params)
    g[:, :D] = (G[:, :D] - mean[None, :] * G[:, W:]) / std[None, :] / n + l2 * w
    g[:, D] = G[:, W] / n
    value = f["totals"][0] / n + 0.5 * l2 * float(np.sum(w * w))
    if not with_bound:
        return float(value), g
    b = np.empty_like(params)
    b[:, :D] = (B[:, :D] + np.abs(mean)[None, :] * B[:, W:]) / std[None, :] / n
    b[:, D] = B[:, W] / n
    return float(value), g, b


def score(x, y, tab, cst):
    """accuracy, balanced accuracy, loss, frames and the confusion table n[truth][prediction], class by class"""
    f = forward(x, y, tab, cst)
    C = f["l"].shape[1]
    conf = np.zeros((C, C))
    for t, q, lab in zip(np.asarray(y), f["pred"], f["labelled"]):
        if lab:
            conf[int(t), int(q)] += 1.0
    n = conf.sum()
    recalls = [conf[c, c] / conf[c].sum() for c in range(C) if conf[c].sum() > 0]
    return {"accuracy": float(np.trace(conf) / n), "balanced_accuracy": float(np.mean(recalls)), "loss": float(f["totals"][0] / n),
            "frames": int(n), "confusion": conf}


# ------------------------------------------------------------------------------------------------------------------ inputs
def case(N, C, D, seed=0, unlabelled=0.1):
    """The inputs of the GPU tests, seeded from (N, C, D): x ~ N(0, 1), tab ~ N(0, 1) / sqrt(D), cst ~ N(0, 1), y uniform over the
    classes with about a tenth of the rows -1 -> (x (N, D) f32, y (N,) int32, tab (C, W) f32, cst (C,) f32)."""
    rng = np.random.default_rng(1000003 * N + 1009 * C + D + 7919 * seed)
    x = rng.standard_normal((N, D)).astype(np.float32)
    tab = np.zeros((C, padded(D)), dtype=np.float32)
    tab[:, :D] = (rng.standard_normal((C, D)) / np.sqrt(D)).astype(np.float32)
    cst = rng.standard_normal(C).astype(np.float32)
    y = rng.integers(0, C, N).astype(np.int32)
    y[rng.random(N) < unlabelled] = -1
    return x, y, tab, cst


def blobs(n_per=600, C=5, D=8, seed=3, spread=2.0):
    """C Gaussian blobs of n_per rows each, interleaved -> (x (N, D) f32, y (N,) int32)"""
    rng = np.random.default_rng(seed)
    centres = spread * rng.standard_normal((C, D))
    y = np.tile(np.arange(C), n_per).astype(np.int32)
    x = (centres[y] + rng.standard_normal((n_per * C, D))).astype(np.float32)
    return x, y
