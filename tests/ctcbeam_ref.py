"""A float64 numpy oracle of include/fhvae_ctcbeam.h, written from the header and not from the kernel: the prefix beam search of
one utterance, vectorised over the classes per frame.  Prefixes are tuples, so identity is by labels by construction.

  decode       one utterance -> (hypothesis, score, decision margin, emptied)
  batch        a CSR batch -> (hyps, scores, margins, status)
  brute_force  the labelling of largest summed path probability (plus the table along the labelling) by enumerating C^T paths

The decision margin is the smallest of: over all frames, the score gap between the last kept and the first dropped candidate;
over all frames, the distance of any finite lp_t[c] from the class-pruning threshold; the gap between the best and the second
best final score.  An implementation whose scores err by less than half the margin takes the same decisions.
"""
import itertools

import numpy as np

from ctc_ref import collapse, log_softmax, lse

EMPTY = 2
NEG = -np.inf


def decode(z, blank, W, table=None, class_beam=np.inf, stats=None):
    """z (T, C) logits -> (hyp list, score, margin, emptied).  stats: a dict whose "recreated" counts the extensions that made a
    prefix one of whose children sat in the beam already (the prefix had fallen out and came back)."""
    z = np.asarray(z)
    T, C = z.shape
    tab = np.zeros((C + 1, C + 1)) if table is None else np.asarray(table, dtype=np.float64)
    margin = np.inf
    beam = [((), 0.0, NEG, 0.0)]  # (prefix, pb, pnb, lm) in beam order
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lp_all = log_softmax(z) if T else np.zeros((0, C))
        for t in range(T):
            lp = lp_all[t]
            thr = lp.max() - class_beam
            is_open = lp >= thr
            fin = np.isfinite(lp)
            if np.isfinite(thr) and fin.any():
                margin = min(margin, float(np.abs(lp[fin] - thr).min()))
            where = {e[0]: i for i, e in enumerate(beam)}
            n = len(beam)
            pb = np.array([e[1] for e in beam])
            pnb = np.array([e[2] for e in beam])
            lmv = np.array([e[3] for e in beam])
            last = np.array([e[0][-1] if e[0] else C for e in beam])
            tot = lse(pb, pnb)
            stay = []  # (pb', pnb') of stay(i)
            excl = np.zeros((n, C), dtype=bool)  # prefix_i + c is in the beam
            for i, (pre, _, _, _) in enumerate(beam):
                spb = tot[i] + lp[blank]
                spnb = pnb[i] + lp[last[i]] if pre else NEG
                if pre and pre[:-1] in where:
                    j = where[pre[:-1]]
                    excl[j, last[i]] = True
                    if is_open[last[i]]:
                        ext = (pb[j] if last[i] == last[j] else tot[j]) + lp[last[i]]
                        spnb = float(lse(spnb, ext))
                stay.append((float(spb), float(spnb)))
            stay_score = lse(np.array([s[0] for s in stay]), np.array([s[1] for s in stay])) + lmv
            # extensions, vectorised over the classes
            base = np.where(np.arange(C)[None, :] == last[:, None], pb[:, None], tot[:, None]) + lp[None, :]  # ext(i, c)
            lm_new = lmv[:, None] + tab[last][:, :C]
            sc = base + lm_new
            ok = is_open[None, :] & ~excl
            ok[:, blank] = False
            sc = np.where(ok, sc, NEG)
            score = np.concatenate([stay_score, sc.reshape(-1)])
            index = np.concatenate([np.arange(n), W + np.arange(n * C)])
            valid = np.nonzero(score > NEG)[0]
            if valid.size == 0:
                return [], NEG, margin, True
            order = valid[np.lexsort((index[valid], -score[valid]))]
            if order.size > W:
                margin = min(margin, float(score[order[W - 1]] - score[order[W]]))
            new = []
            for o in order[:W]:
                if o < n:
                    new.append((beam[o][0], stay[o][0], stay[o][1], lmv[o]))
                else:
                    i, c = divmod(int(o) - n, C)
                    new.append((beam[i][0] + (c,), NEG, float(base[i, c]), float(lm_new[i, c])))
            if stats is not None:
                made = {e[0] for o, e in zip(order[:W], new) if o >= n}
                stats["recreated"] = stats.get("recreated", 0) + sum(1 for e in new if e[0] and e[0][:-1] in made)
            beam = new
        final = [(float(lse(e[1], e[2])) + e[3]) + tab[e[0][-1] if e[0] else C][C] for e in beam]
    best = 0
    for i in range(1, len(final)):
        if final[i] > final[best]:
            best = i
    if len(final) > 1:
        rest = max(f for i, f in enumerate(final) if i != best)
        if np.isfinite(final[best]):
            margin = min(margin, final[best] - rest)
    return list(beam[best][0]), float(final[best]), float(margin), False


def batch(z, utt_ptr, blank, W, table=None, class_beam=np.inf):
    """-> (hyps: list of lists, scores (U,), margins (U,), status)."""
    U = len(utt_ptr) - 1
    hyps, scores, margins, status = [], np.zeros(U), np.zeros(U), 0
    for u in range(U):
        h, s, m, emptied = decode(np.asarray(z)[int(utt_ptr[u]):int(utt_ptr[u + 1])], blank, W, table, class_beam)
        hyps.append(h)
        scores[u], margins[u] = s, m
        status |= EMPTY if emptied else 0
    return hyps, scores, margins, status


def brute_force(z, blank, table=None):
    """Every labelling's log of the summed probability of its paths, plus the table along it (start, pairs, end) ->
    {labelling tuple: score}; z (T, C) with T <= 5 or so."""
    z = np.asarray(z, dtype=np.float64)
    T, C = z.shape
    tab = np.zeros((C + 1, C + 1)) if table is None else np.asarray(table, dtype=np.float64)
    p = np.exp(log_softmax(z)) if T else np.zeros((0, C))
    mass = {}
    for path in itertools.product(range(C), repeat=T):
        lab = tuple(collapse(path, blank))
        mass[lab] = mass.get(lab, 0.0) + float(np.prod([p[t, c] for t, c in enumerate(path)]))
    out = {}
    with np.errstate(divide="ignore"):
        for lab, m in mass.items():
            prev, add = C, 0.0
            for v in lab:
                add += tab[prev][v]
                prev = v
            out[lab] = float(np.log(m)) + (add + tab[prev][C])
    return out
