"""A scalar numpy oracle of include/fhvae_abx.h and of abx.abx_scores: frame costs in float64 rounded once to f32, the DTW
recursion cell by cell in np.float32 with the stated tie order, and ABX as a literal loop over triples."""
import numpy as np


def frame_costs(a, b, metric):
    """a (n, D), b (m, D) f32 -> (n, m) f32 costs.  float64 products and sums in increasing k."""
    a64, b64 = np.asarray(a, dtype=np.float32).astype(np.float64), np.asarray(b, dtype=np.float32).astype(np.float64)
    n, m, D = a64.shape[0], b64.shape[0], a64.shape[1]
    dot, na2, nb2 = np.zeros((n, m)), np.zeros(n), np.zeros(m)
    for k in range(D):  # (np.dot would sum in another order)
        dot = dot + a64[:, k, None] * b64[None, :, k]
        na2 = na2 + a64[:, k] * a64[:, k]
        nb2 = nb2 + b64[:, k] * b64[:, k]
    na, nb = np.sqrt(na2), np.sqrt(nb2)
    den = na[:, None] * nb[None, :]
    zero = (na[:, None] == 0) | (nb[None, :] == 0)
    cos = np.clip(dot / np.where(zero, 1.0, den), -1.0, 1.0)
    cos = np.where(zero, 0.0, cos)
    c = np.arccos(cos) / np.pi if metric == "angular" else 1.0 - cos
    return c.astype(np.float32)


def dtw(a, b, metric):
    """-> (d, gap): the path-length-normalised DTW cost as np.float32, and the smallest difference between the chosen and the
    next-best predecessor over the cells of the optimal path, relative to D[n - 1][m - 1] (inf when no cell had a choice)."""
    c = frame_costs(a, b, metric)
    n, m = c.shape
    D = np.zeros((n, m), dtype=np.float32)
    L = np.zeros((n, m), dtype=np.int64)
    choice = np.zeros((n, m), dtype=np.int64)  # 0 diagonal, 1 up, 2 left
    margin = np.full((n, m), np.inf)
    for i in range(n):
        for j in range(m):
            if i == 0 and j == 0:
                D[0, 0], L[0, 0] = c[0, 0], 1
                continue
            if i == 0:
                pd, pl, ch = D[0, j - 1], L[0, j - 1], 2
            elif j == 0:
                pd, pl, ch = D[i - 1, 0], L[i - 1, 0], 1
            else:
                cand = [(D[i - 1, j - 1], L[i - 1, j - 1]), (D[i - 1, j], L[i - 1, j]), (D[i, j - 1], L[i, j - 1])]
                ch = 0
                if cand[1][0] < cand[ch][0]:
                    ch = 1
                if cand[2][0] < cand[ch][0]:
                    ch = 2
                pd, pl = cand[ch]
                margin[i, j] = min(float(x[0]) - float(pd) for k, x in enumerate(cand) if k != ch)
            D[i, j] = np.float32(pd) + c[i, j]  # (np.float32 + np.float32: one rounding)
            L[i, j] = pl + 1
            choice[i, j] = ch
    gap, i, j = np.inf, n - 1, m - 1
    while i > 0 or j > 0:
        gap = min(gap, margin[i, j])
        i, j = (i - 1, j - 1) if choice[i, j] == 0 else ((i - 1, j) if choice[i, j] == 1 else (i, j - 1))
    total = float(D[n - 1, m - 1])
    return np.float32(D[n - 1, m - 1] / np.float32(L[n - 1, m - 1])), (gap / total if total > 0 else np.inf)


def group_matrix(feats, start, length, metric):
    """The dense (n, n) block of one group -> (block f32, gaps (n, n) with inf on the diagonal)."""
    n = len(start)
    out, gaps = np.zeros((n, n), dtype=np.float32), np.full((n, n), np.inf)
    for i in range(n):
        for j in range(i + 1, n):
            d, g = dtw(feats[start[i]:start[i] + length[i]], feats[start[j]:start[j] + length[j]], metric)
            out[i, j] = out[j, i] = d
            gaps[i, j] = gaps[j, i] = g
    return out, gaps


def abx_triples(dist, phone, ctx, spk):
    """dist(a, b) -> the distance between tokens a and b.  The literal ABX of abx.abx_scores: a loop over every triple.
    Returns {"within", "across", "cells_*", "triples_*", "gt_*", "eq_*", "compared": the (d(A, X), d(B, X)) of every triple}."""
    N = len(phone)
    res, compared = {}, []
    for task in ("within", "across"):
        cells = {}
        for A in range(N):
            for X in range(N):
                if A == X or phone[A] != phone[X] or ctx[A] != ctx[X]:
                    continue
                if (spk[A] == spk[X]) != (task == "within"):
                    continue
                for B in range(N):
                    if ctx[B] != ctx[A] or spk[B] != spk[A] or phone[B] == phone[A]:
                        continue
                    key = (phone[A], phone[B], ctx[A], spk[A]) + ((spk[X],) if task == "across" else ())
                    cell = cells.setdefault(key, [0, 0, 0])
                    dax, dbx = dist(A, X), dist(B, X)
                    compared.append((dax, dbx))
                    cell[0] += 1
                    cell[1] += int(dax > dbx)
                    cell[2] += int(dax == dbx)
        by_pair = {}
        for key, (n, gt, eq) in cells.items():
            by_pair.setdefault(key[:2], []).append((gt + 0.5 * eq) / n)
        pair_means = [np.mean(v) for v in by_pair.values()]
        res[task] = float(np.mean(pair_means)) if pair_means else float("nan")
        res["cells_" + task] = len(cells)
        res["triples_" + task] = sum(v[0] for v in cells.values())
        res["gt_" + task] = sum(v[1] for v in cells.values())
        res["eq_" + task] = sum(v[2] for v in cells.values())
    res["compared"] = compared
    return res
