"""The oracle of units.py and csrc/kmeans.hip, in numpy float64 and plain loops: the all-pairs scores, the error bound of the f32
kernel, the centroid update in the piece order of include/fhvae_kmeans.h (bit for bit what the kernels must give), Lloyd's
algorithm with units.fit's init / reseed / stop rules, and the quality metrics and the bitrate as literal loops."""
import math

import numpy as np

PIECE = 256


# ------------------------------------------------------------------------------------------------------------------ assign
def scores(x, cent):
    """-> (s64 (N, K), xn64 (N,)): s64(n, k) = |c_k|^2 - 2 x_n . c_k in float64; |x_n - c_k|^2 = xn64[n] + s64[n][k]."""
    x, cent = np.asarray(x, dtype=np.float64), np.asarray(cent, dtype=np.float64)
    return (cent * cent).sum(axis=1)[None, :] - 2.0 * (x @ cent.T), (x * x).sum(axis=1)


def bound(x, cent):
    """E(n) = 2^-23 (D + 1) (|x_n|^2 + max_k |c_k|^2): what the f32 chains of length D plus one rounding can move a score by."""
    x, cent = np.asarray(x, dtype=np.float64), np.asarray(cent, dtype=np.float64)
    return 2.0 ** -23 * (x.shape[1] + 1) * ((x * x).sum(axis=1) + (cent * cent).sum(axis=1).max())


def assign(x, cent):
    """-> (labels (the first of equal float64 scores), d64 = max(xn + min score, 0), gap: runner-up score minus the best (inf
    when K = 1), E)."""
    s, xn = scores(x, cent)
    labels = s.argmin(axis=1)
    best = s[np.arange(s.shape[0]), labels]
    if s.shape[1] > 1:
        gap = np.partition(s, 1, axis=1)[:, 1] - best
    else:
        gap = np.full(s.shape[0], np.inf)
    return labels.astype(np.int32), np.maximum(xn + best, 0.0), gap, bound(x, cent)


# ------------------------------------------------------------------------------------------------------------------ update
def two_level_sum(values):
    """values (n, ...) -> their sum in float64: pieces of PIECE consecutive entries summed in order from 0, the piece sums added
    in order from 0."""
    values = np.asarray(values)
    total = np.zeros(values.shape[1:], dtype=np.float64)
    for p0 in range(0, values.shape[0], PIECE):
        piece = np.zeros(values.shape[1:], dtype=np.float64)
        for v in values[p0:p0 + PIECE]:
            piece = piece + v.astype(np.float64)
        total = total + piece
    return total


def update(x, labels, cent, dist=None):
    """-> (new centroids f32 (a cluster without members keeps its row), counts int64, cl_inertia float64)."""
    x, labels = np.asarray(x, dtype=np.float32), np.asarray(labels)
    new = np.array(cent, dtype=np.float32, copy=True)
    K = new.shape[0]
    counts, inertia = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.float64)
    for k in range(K):
        rows = np.nonzero(labels == k)[0]  # (increasing row index)
        counts[k] = rows.shape[0]
        if rows.shape[0] == 0:
            continue
        new[k] = (two_level_sum(x[rows]) / np.float64(rows.shape[0])).astype(np.float32)
        if dist is not None:
            inertia[k] = two_level_sum(np.asarray(dist)[rows])
    return new, counts, inertia


# ------------------------------------------------------------------------------------------------------------------- Lloyd
def reseed(labels, dist, counts):
    """In place: the empty clusters, in increasing k, take the rows of largest dist (equal ones: the smaller row first)."""
    empty = np.nonzero(counts == 0)[0]
    if empty.shape[0]:
        far = np.argsort(-np.asarray(dist, dtype=np.float64), kind="stable")[:empty.shape[0]]
        labels[far] = empty
    return int(empty.shape[0])


def lloyd(x, init, iters, tol=1e-4):
    """units.fit from `init` with float64 scores.  -> a list with one dict per iteration: labels (after reseeding), centroids
    (after the update, f32), inertia, min_margin (the smallest over the rows of gap - 2 E, before reseeding: positive means the
    f32 kernel must give these labels), reseeded, and "converged" in the last one."""
    x = np.asarray(x, dtype=np.float32)
    cent = np.array(init, dtype=np.float32, copy=True)
    K = cent.shape[0]
    hist, prev, prev_inertia = [], None, None
    for _ in range(iters):
        labels, d64, gap, E = assign(x, cent)
        counts = np.bincount(labels, minlength=K)
        e = reseed(labels, d64, counts)
        changed = prev is None or bool((labels != prev).any())
        cent, counts, cl_inertia = update(x, labels, cent, d64)
        inertia = float(np.sum(cl_inertia, dtype=np.float64))
        done = (not changed) or (prev_inertia is not None and prev_inertia - inertia < tol * prev_inertia)
        hist.append({"labels": labels.copy(), "centroids": cent.copy(), "inertia": inertia, "min_margin": float((gap - 2 * E).min()),
                     "reseeded": e > 0, "counts": counts, "converged": done})
        prev, prev_inertia = labels, inertia
        if done:
            break
    return hist


# ----------------------------------------------------------------------------------------------------------------- metrics
def unit_quality(labels, phones, k):
    """cluster purity, phone purity, PNMI and the labelled frames, entry by entry."""
    P = max([int(p) for p in phones] + [-1]) + 1
    table = [[0] * P for _ in range(k)]
    n = 0
    for u, p in zip(labels, phones):
        if p >= 0:
            table[int(u)][int(p)] += 1
            n += 1
    if n == 0:
        return {"cluster_purity": 0.0, "phone_purity": 0.0, "pnmi": 0.0, "labelled_frames": 0}
    row = [sum(r) for r in table]
    col = [sum(table[u][p] for u in range(k)) for p in range(P)]
    cp = sum(max(r) for r in table if r) / n
    pp = sum(max(table[u][p] for u in range(k)) for p in range(P)) / n
    mi = sum(table[u][p] / n * math.log(table[u][p] * n / (row[u] * col[p])) for u in range(k) for p in range(P) if table[u][p])
    hp = -sum(c / n * math.log(c / n) for c in col if c)
    return {"cluster_purity": cp, "phone_purity": pp, "pnmi": mi / hp if hp > 0 else 0.0, "labelled_frames": n}


def bitrate(seqs, frame_shift):
    """M H / duration for the sequences and for their run-length collapsed forms."""
    def bits(ss, duration):
        count, m = {}, 0
        for s in ss:
            for u in s:
                count[int(u)] = count.get(int(u), 0) + 1
                m += 1
        if m == 0:
            return 0.0
        h = -sum(c / m * math.log2(c / m) for c in count.values())
        return m * h / duration

    frames = sum(len(s) for s in seqs)
    if frames == 0:
        return {"bitrate": 0.0, "bitrate_collapsed": 0.0}
    collapsed = [[u for j, u in enumerate(s) if j == 0 or u != s[j - 1]] for s in seqs]
    return {"bitrate": bits(seqs, frames * frame_shift), "bitrate_collapsed": bits(collapsed, frames * frame_shift)}
