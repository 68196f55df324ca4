"""A scalar numpy float64 oracle of include/fhvae_falign.h, written from the header and not from the kernel: the max-plus
recursion of one utterance state by state, the back-pointers with the header's tie rule (the smallest k of the largest
candidate), the end rule (equal values go to S - 1) and the trace-back.

  extended     the states' classes l' and the skip mask of a transcription, for either topology (blank == -1: HMM)
  align        one utterance -> (state (T,) int32, seg (L, 2) int32, score float64, flag)
  batch        a CSR batch -> (state (N,), seg (2 sum L,), score (U,), status)
  brute_force  every state path of the topology: the largest float64 sum and, among the paths that reach it, the first one in
               the tie order of the back-pointers
  collapse     the classes of a state path with the runs of a state merged and the blank dropped
"""
import itertools

import numpy as np

BAD_LABEL, INFEASIBLE = 2, 4
MAX_LABELS = 256
NEG = -np.inf


def extended(labels, blank):
    """-> (ext (S,) int64: l'_s, skip (S,) bool: whether the step s - 2 -> s is allowed, the start states, the end states in the
    order of preference)."""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    L = labels.shape[0]
    if blank < 0:
        return labels.copy(), np.zeros(L, dtype=bool), [0], [L - 1]
    S = 2 * L + 1
    ext = np.full(S, blank, dtype=np.int64)
    ext[1::2] = labels
    skip = np.zeros(S, dtype=bool)
    skip[3::2] = labels[1:] != labels[:-1]
    return ext, skip, [0, 1], ([S - 1, S - 2] if L >= 1 else [S - 1])


def align(z, labels, blank):
    """z (T, C) f32 scores, labels a sequence of ints, blank in [0, C) or -1 -> (state (T,) int32, seg (L, 2) int32, score, flag)."""
    z = np.asarray(z, dtype=np.float32)
    T, C = z.shape
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    L = labels.shape[0]
    none = (np.full(T, -1, dtype=np.int32), np.full((L, 2), -1, dtype=np.int32), NEG)
    if L > MAX_LABELS or (L and (labels.min() < 0 or labels.max() >= C or (blank >= 0 and (labels == blank).any()))):
        return none + (BAD_LABEL,)
    if T == 0:
        return (none[0], none[1], 0.0, 0) if L == 0 else none + (INFEASIBLE,)
    ext, skip, starts, ends = extended(labels, blank)
    S = ext.shape[0]
    if S == 0:
        return none + (INFEASIBLE,)
    delta = np.full(S, NEG)
    for s in starts:
        if s < S:
            delta[s] = np.float64(z[0, ext[s]])
    back = np.zeros((T, S), dtype=np.int8)
    e = z[:, ext].astype(np.float64)  # (T, S): e_t(s), exact
    cols = np.arange(S)
    pad1, pad2 = np.full(1, NEG), np.full(2, NEG)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):  # the states of a frame side by side; the frames one after the other
            cand = np.stack([delta, np.concatenate([pad1, delta[:-1]]), np.where(skip, np.concatenate([pad2, delta[:-2]])[:S], NEG)])
            k = np.argmax(cand, axis=0)  # the first, that is the smallest, k of the largest candidate (all -inf: 0)
            back[t] = k
            delta = cand[k, cols] + e[t]
    q = ends[0]
    for s in ends[1:]:
        if delta[s] > delta[q]:
            q = s
    score = float(delta[q])
    if score == NEG:
        return none + (INFEASIBLE,)
    state = np.zeros(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        state[t] = q
        q = max(q - int(back[t, q]), 0)
    seg = np.full((L, 2), -1, dtype=np.int32)
    for i in range(L):
        at = np.nonzero(state == (2 * i + 1 if blank >= 0 else i))[0]
        if at.size:
            seg[i] = (at[0], at[-1])
    return state, seg, score, 0


def batch(z, utt_ptr, labels, lab_ptr, blank):
    """-> (state (N,) int32, seg (2 lab_ptr[-1],) int32, score (U,) float64, status)."""
    z = np.asarray(z, dtype=np.float32)
    U = len(utt_ptr) - 1
    state = np.zeros(z.shape[0], dtype=np.int32)
    seg = np.zeros(2 * int(lab_ptr[-1]), dtype=np.int32)
    score = np.zeros(U)
    status = 0
    for u in range(U):
        a, b, la, lb = int(utt_ptr[u]), int(utt_ptr[u + 1]), int(lab_ptr[u]), int(lab_ptr[u + 1])
        state[a:b], sg, score[u], flag = align(z[a:b], labels[la:lb], blank)
        seg[2 * la:2 * lb] = sg.reshape(-1)
        status |= flag
    return state, seg, score, status


def collapse(state, labels, blank):
    """The classes along a state path, runs of one STATE merged, the blank dropped."""
    ext = extended(labels, blank)[0]
    out, last = [], None
    for q in state:
        if q != last and (blank < 0 or ext[q] != blank):
            out.append(int(ext[q]))
        last = q
    return out


def brute_force(z, labels, blank):
    """Every state path of the topology (T and S small) -> (score, state path): the largest sum, added in increasing t in float64
    as the recursion does; among equal sums the path whose LAST state is the preferred end state, then whose back-pointers are
    smallest from the last frame backwards, which is what the header's tie rules give.  (-inf, None) if no path is finite."""
    z = np.asarray(z, dtype=np.float32)
    T = z.shape[0]
    ext, skip, starts, ends = extended(labels, blank)
    S = ext.shape[0]
    best, arg = None, None
    if T == 0 or S == 0:
        return (0.0, ()) if (T == 0 and len(labels) == 0) else (NEG, None)
    for path in itertools.product(range(S), repeat=T):
        if path[0] not in starts or path[-1] not in ends:
            continue
        steps = [b - a for a, b in zip(path[:-1], path[1:])]
        if any(d < 0 or d > 2 or (d == 2 and not skip[b]) for d, b in zip(steps, path[1:])):
            continue
        total = np.float64(z[0, ext[path[0]]])
        for t in range(1, T):
            total = total + np.float64(z[t, ext[path[t]]])
        if total == NEG:
            continue
        key = (-float(total), ends.index(path[-1]), tuple(steps[::-1]))
        if best is None or key < best:
            best, arg = key, path
    return (NEG, None) if best is None else (-best[0], arg)
