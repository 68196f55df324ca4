"""Scalar numpy oracles of include/fhvae_viterbi.h and of phonerec.transitions, and the generator of the synthetic phone corpus.

  decode       the Viterbi recursion of the header to the letter: f32, one rounding per addition, the smallest index of equal maxima
  align        the Levenshtein cells (cost, S, D, I, Cor) of the header, cell by cell, ties to diagonal, up, left in that order
  align_fast   the same cells walked by anti-diagonals in numpy (for the long pairs of the GPU grid; test_phonerec_cpu pins it
               to `align`)
  transitions  the frame-level bigram, frame by frame
  corpus       Gaussian blobs per phone, utterances of a few phones of a few frames each
"""
import numpy as np

NEG = np.float32(-np.inf)


def decode(emit, trans, init, fin=None):
    """One utterance: emit (m, C) f32 -> (path (m,) int32, score f32).  m = 0: (empty, -inf)."""
    emit, trans, init = np.asarray(emit, np.float32), np.asarray(trans, np.float32), np.asarray(init, np.float32)
    m, C = emit.shape
    if m == 0:
        return np.zeros(0, np.int32), NEG
    with np.errstate(invalid="ignore"):
        d = init + emit[0]
        back = np.zeros((m, C), dtype=np.int32)
        for t in range(1, m):
            v = d[:, None] + trans          # v[p][c], f32, one rounding
            b = np.argmax(v, axis=0)        # the first, that is the smallest, p of the largest v (all -inf: 0)
            back[t] = b
            d = v[b, np.arange(C)] + emit[t]
        w = d if fin is None else d + np.asarray(fin, np.float32)
    q = int(np.argmax(w))
    path = np.zeros(m, dtype=np.int32)
    path[m - 1] = q
    for t in range(m - 1, 0, -1):
        q = int(back[t][q])
        path[t - 1] = q
    return path, np.float32(w[path[m - 1]])


def decode_batch(emit, utt_ptr, trans, init, fin=None):
    """-> (path (n_frames,) int32, score (U,) f32) of a CSR batch."""
    emit = np.asarray(emit, np.float32)
    path = np.zeros(emit.shape[0], dtype=np.int32)
    score = np.zeros(len(utt_ptr) - 1, dtype=np.float32)
    for u, (a, b) in enumerate(zip(utt_ptr[:-1], utt_ptr[1:])):
        path[a:b], score[u] = decode(emit[a:b], trans, init, fin)
    return path, score


def brute_force(emit, trans, init, fin=None):
    """The maximum over all C^m paths in float64 (exact on integer-valued inputs); equal scores: the path whose LAST state is
    smallest, then the one whose predecessor is smallest and so on backwards, which is what the back-pointers' tie rule gives."""
    import itertools

    m, C = emit.shape
    best, arg = None, None
    for q in itertools.product(range(C), repeat=m):
        s = float(init[q[0]]) + float(emit[0][q[0]])
        for t in range(1, m):
            s += float(trans[q[t - 1]][q[t]]) + float(emit[t][q[t]])
        if fin is not None:
            s += float(fin[q[-1]])
        key = (-s, q[::-1])
        if best is None or key < best:
            best, arg = key, q
    return np.asarray(arg, dtype=np.int32), -best[0]


def align(ref, hyp):
    """-> (S, D, I, Cor) of the header's cell [|ref|][|hyp|], cell by cell."""
    n, m = len(ref), len(hyp)
    row = [(j, 0, 0, j, 0) for j in range(m + 1)]
    for i in range(1, n + 1):
        new = [(i, 0, i, 0, 0)]
        for j in range(1, m + 1):
            dg, up, lf = row[j - 1], row[j], new[j - 1]
            ne = int(ref[i - 1] != hyp[j - 1])
            best = (dg[0] + ne, dg[1] + ne, dg[2], dg[3], dg[4] + 1 - ne)
            if up[0] + 1 < best[0]:
                best = (up[0] + 1, up[1], up[2] + 1, up[3], up[4])
            if lf[0] + 1 < best[0]:
                best = (lf[0] + 1, lf[1], lf[2], lf[3] + 1, lf[4])
            new.append(best)
        row = new
    return tuple(int(v) for v in row[m][1:])


def align_fast(ref, hyp):
    """`align` with the cells of one anti-diagonal i + j = k computed together."""
    ref, hyp = np.asarray(ref, dtype=np.int64), np.asarray(hyp, dtype=np.int64)
    n, m = len(ref), len(hyp)
    if n == 0 or m == 0:
        return (0, n, m, 0)
    # cell[i][j] of diagonal k lives at index i of an (n + 1, 5) array
    cur = np.zeros((n + 1, 5), dtype=np.int64)
    prev = np.zeros((n + 1, 5), dtype=np.int64)   # diagonal k - 1
    prev2 = np.zeros((n + 1, 5), dtype=np.int64)  # diagonal k - 2
    prev2[0] = (0, 0, 0, 0, 0)                    # k = 0
    prev[0], prev[1] = (1, 0, 0, 1, 0), (1, 0, 1, 0, 0)  # k = 1: [0][1], [1][0]
    for k in range(2, n + m + 1):
        lo, hi = max(0, k - m), min(n, k)
        cur[:] = 0
        if lo == 0:
            cur[0] = (k, 0, 0, k, 0)
        if hi == k:
            cur[k] = (k, 0, k, 0, 0)
        i = np.arange(max(lo, 1), min(hi, k - 1) + 1)
        if i.size:
            j = k - i
            ne = (ref[i - 1] != hyp[j - 1]).astype(np.int64)
            dg, up, lf = prev2[i - 1], prev[i - 1], prev[i]
            best = dg.copy()
            best[:, 0] += ne
            best[:, 1] += ne
            best[:, 4] += 1 - ne
            c = up.copy()
            c[:, 0] += 1
            c[:, 2] += 1
            take = c[:, 0] < best[:, 0]
            best[take] = c[take]
            c = lf.copy()
            c[:, 0] += 1
            c[:, 3] += 1
            take = c[:, 0] < best[:, 0]
            best[take] = c[take]
            cur[i] = best
        prev2, prev, cur = prev, cur, prev2
    return tuple(int(v) for v in prev[n][1:])


def levenshtein(ref, hyp):
    """The plain edit distance, two rows."""
    row = list(range(len(hyp) + 1))
    for i, r in enumerate(ref, 1):
        new = [i]
        for j, h in enumerate(hyp, 1):
            new.append(min(row[j - 1] + (r != h), row[j] + 1, new[j - 1] + 1))
        row = new
    return row[-1]


def transitions(labels, lengths, n_classes, smooth=1.0, penalty=0.0):
    """phonerec.transitions frame by frame -> (trans (C, C) f32, init (C,) f32)."""
    pair = np.zeros((n_classes, n_classes))
    first = np.zeros(n_classes)
    a = 0
    for n in lengths:
        seen = False
        for t in range(a, a + n):
            if labels[t] < 0:
                continue
            if not seen:
                first[labels[t]] += 1
                seen = True
            if t > a and labels[t - 1] >= 0:
                pair[labels[t - 1]][labels[t]] += 1
        a += n
    trans = np.zeros((n_classes, n_classes))
    for p in range(n_classes):
        row = pair[p] + smooth
        row = row if row.sum() > 0 else np.ones(n_classes)
        with np.errstate(divide="ignore"):
            trans[p] = np.log(row / row.sum())
        for c in range(n_classes):
            if c != p:
                trans[p][c] -= penalty
    f = first + smooth
    f = f if f.sum() > 0 else np.ones(n_classes)
    with np.errstate(divide="ignore"):
        init = np.log(f / f.sum())
    return trans.astype(np.float32), init.astype(np.float32)


def collapse(seq):
    return [int(v) for i, v in enumerate(seq) if i == 0 or v != seq[i - 1]]


def corpus(n_utts=60, n_phones=5, D=8, sigma=1.3, seed=0):
    """Gaussian blobs: phone p has mean means[p] (standard normal entries) and covariance sigma^2 I.  Every utterance holds 4 to
    8 phones (neighbours differ) of 3 to 10 frames each.
    -> {"x" (N, D) f32, "y" (N,) int32, "lengths" (U,) int64, "refs" list of int lists, "means" (P, D) float64, "sigma"}"""
    rng = np.random.RandomState(seed)
    means = rng.standard_normal((n_phones, D))
    xs, ys, lengths, refs = [], [], [], []
    for _ in range(n_utts):
        phones, last = [], -1
        for _ in range(rng.randint(4, 9)):
            p = rng.randint(n_phones - (last >= 0))
            p += int(last >= 0 and p >= last)
            phones.append(int(p))
            last = p
        y = np.concatenate([np.full(rng.randint(3, 11), p, dtype=np.int32) for p in phones])
        xs.append(means[y] + sigma * rng.standard_normal((y.shape[0], D)))
        ys.append(y), lengths.append(y.shape[0]), refs.append(phones)
    return {"x": np.concatenate(xs).astype(np.float32), "y": np.concatenate(ys), "lengths": np.asarray(lengths, dtype=np.int64),
            "refs": refs, "means": means, "sigma": float(sigma)}


def log_posteriors(x, means, sigma):
    """The true model's log p(phone | x) under equal priors, float64 -> f32."""
    d2 = ((x[:, None, :].astype(np.float64) - means[None]) ** 2).sum(axis=2)
    l = -0.5 * d2 / sigma ** 2
    l -= l.max(axis=1, keepdims=True)
    return (l - np.log(np.exp(l).sum(axis=1, keepdims=True))).astype(np.float32)


def per(refs, hyps, fast=False):
    """The phone error rate of hypothesis lists against reference lists, by `align`."""
    tot = np.zeros(4, dtype=np.int64)
    for r, h in zip(refs, hyps):
        tot += np.asarray((align_fast if fast else align)(r, h))
    S, Dl, I, Cor = tot
    return float(S + Dl + I) / float(S + Dl + Cor)
