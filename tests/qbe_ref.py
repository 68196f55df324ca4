"""A scalar numpy oracle of include/fhvae_qbe.h and of qbe.rank_metrics: the frame costs of abx_ref, the subsequence-DTW
recursion cell by cell in np.float32 with the stated tie order, and the ranking scores as a literal loop."""
import numpy as np

import abx_ref


def sdtw(q, u, metric):
    """q (n, D), u (m, D), m >= 1 -> (e (m,) f32, s (m,) int64, gap (m,)): per end column j the length-normalised cost of the
    best alignment of the whole query that ends there, the frame it starts at, and the smallest difference between the chosen
    and the next-best predecessor over the cells of that column's path, relative to D[n - 1][j] (inf when no cell had a
    choice)."""
    c = abx_ref.frame_costs(q, u, metric)
    n, m = c.shape
    D = np.zeros((n, m), dtype=np.float32)
    L = np.zeros((n, m), dtype=np.int64)
    S = np.zeros((n, m), dtype=np.int64)
    G = np.full((n, m), np.inf)  # the smallest margin on the path into (i, j)
    for i in range(n):
        for j in range(m):
            if i == 0:
                D[0, j], L[0, j], S[0, j] = c[0, j], 1, j
                continue
            if j == 0:
                pd, pl, ps, pg = D[i - 1, 0], L[i - 1, 0], S[i - 1, 0], G[i - 1, 0]
            else:
                cand = [(i - 1, j - 1), (i - 1, j), (i, j - 1)]
                ch = 0
                if D[cand[1]] < D[cand[ch]]:
                    ch = 1
                if D[cand[2]] < D[cand[ch]]:
                    ch = 2
                pd, pl, ps = D[cand[ch]], L[cand[ch]], S[cand[ch]]
                pg = min(G[cand[ch]], min(float(D[x]) - float(pd) for k, x in enumerate(cand) if k != ch))
            D[i, j] = np.float32(pd) + c[i, j]  # (np.float32 + np.float32: one rounding)
            L[i, j], S[i, j], G[i, j] = pl + 1, ps, pg
    e = (D[n - 1] / L[n - 1].astype(np.float32)).astype(np.float32)
    total = D[n - 1].astype(np.float64)
    gap = np.where(total > 0, G[n - 1] / np.where(total > 0, total, 1.0), np.inf)
    return e, S[n - 1].copy(), gap


def best(e):
    """-> (the smallest j that minimises e, e[j])"""
    j = 0
    for k in range(1, len(e)):
        if e[k] < e[j]:
            j = k
    return j, e[j]


def rank_metrics(best_cost, best_start, best_end, q_term, q_utt, truth, same_corpus=True):
    """The literal loop of qbe.rank_metrics.  q_term: the term's name per query, q_utt: its utterance; truth: a list of
    (utt, first, last, term)."""
    Q, U = len(best_cost), len(best_cost[0])
    aps, pns, p10s, found, pairs, no_target = [], [], [], 0, 0, 0
    for q in range(Q):
        cand = [u for u in range(U) if not (same_corpus and u == q_utt[q])]
        rel = [u for u in cand if any(t[0] == u and t[3] == q_term[q] for t in truth)]
        if not rel:
            no_target += 1
            continue
        ranked = sorted(cand, key=lambda u: (float(best_cost[q][u]), u))
        hits, ap = 0, 0.0
        for r, u in enumerate(ranked, 1):
            if u in rel:
                hits += 1
                ap += hits / r
        aps.append(ap / len(rel))
        pns.append(sum(1 for u in ranked[:len(rel)] if u in rel) / len(rel))
        K = min(10, len(ranked))
        p10s.append(sum(1 for u in ranked[:K] if u in rel) / K)
        for u in rel:
            d0, d1 = int(best_start[q][u]), int(best_end[q][u])
            ok = False
            for tu, f, l, term in truth:
                if tu == u and term == q_term[q] and d1 >= 0:
                    over = min(d1, l) - max(d0, f) + 1
                    ok = ok or 2 * over >= min(d1 - d0 + 1, l - f + 1)
            found += int(ok)
            pairs += 1
    mean = lambda v: sum(v) / len(v) if v else None
    return {"map": mean(aps), "p_at_n": mean(pns), "p_at_10": mean(p10s), "located": found / pairs if pairs else None,
            "queries": len(aps), "no_target": no_target}
