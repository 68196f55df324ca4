"""The oracle of segment.py and csrc/segment.hip (include/fhvae_segment.h), in numpy float64 and plain loops: the cells' scores
and their error bound, the dynamic programme with the header's tie rule (bit for bit what the kernel must give on the same
scores), the objective J64 of any segmentation, and a brute force over all cuts.

THE BOUND B(n, l) on |score_device - score64|.  With u = 2^-24, S the float64 segment sum (its own error, l 2^-53 |S|, is far
below what follows), c a centroid, and s64 = l |c|^2 - 2 S . c:
  Sf  = (float)S                     |Sf . c - S . c|  <= u |S| |c|                        one rounding of S to f32
  dot = the fmaf chain of length D   |dot - Sf . c|    <= g_D |Sf| |c|,  g_D = D u / (1 - D u)
  cn  = the fmaf chain of length D   |cn - |c|^2|      <= g_D |c|^2
  p   = (float)l * cn, one rounding  |p - l |c|^2|     <= g_{D+1} l |c|^2
  s   = fmaf(-2, dot, p), one rounding: s = (p - 2 dot)(1 + d), |d| <= u
so  |s - s64| <= u |p - 2 dot| + 2 |dot - S . c| + |p - l |c|^2|
              <= u (l |c|^2 + 2 |S| |c|) (1 + g) + 2 (u + g_D (1 + u)) |S| |c| + g_{D+1} l |c|^2
              <= u (1 + e) [ (2 D + 4) |S| |c| + (D + 2) l |c|^2 ]          (e of the order D u <= 2^-17)
and with 2 |S| |c| <= |S|^2 / l + l |c|^2:
              <= u (1 + e) (D + 2) [ |S|^2 / l + 2 l |c|^2 ]  <=  2^-23 (D + 2) ( |S|^2 / l + l max_k |c_k|^2 ) = B(n, l).
The last step doubles the |S|^2 / l term, which pays for e many times over.  The minimum over k moves by at most the largest
move of a score, so the bound holds for score = min_k s with max_k |c_k|^2.  It is derived, not fitted to device output.
"""
import itertools
import math

import numpy as np

BAD_PTR, NOT_FINITE = 1, 2
MAX_LEN = 64


# ------------------------------------------------------------------------------------------------------------------ scores
def segment_sums(x, max_len):
    """x (T, D) of ONE utterance -> S64 (T, max_len, D): S64[n][l-1] = x[n] + x[n-1] + .. + x[n-l+1] added in that order from 0 in
    float64; rows with l > n + 1 are NaN (no such segment)."""
    x = np.asarray(x, dtype=np.float32)
    T, D = x.shape
    S = np.full((T, max_len, D), np.nan, dtype=np.float64)
    for n in range(T):
        acc = np.zeros(D, dtype=np.float64)
        for l in range(1, min(max_len, n + 1) + 1):
            acc = acc + x[n - l + 1].astype(np.float64)
            S[n, l - 1] = acc
    return S


def scores_loops(x, cent, max_len):
    """One utterance -> (score64 (T, max_len) float64, unit (T, max_len) int32, gap (T, max_len): runner-up minus best, inf with
    K = 1, B (T, max_len)), every cell and every unit in a literal loop.  A segment that crosses the start has score +inf, unit
    -1, gap inf, B 0.  A score that is NaN never wins; a cell with nothing but NaN has score +inf and unit 0."""
    x, cent = np.asarray(x, dtype=np.float32), np.asarray(cent, dtype=np.float32)
    T, D = x.shape
    K = cent.shape[0]
    c64 = cent.astype(np.float64)
    cn = (c64 * c64).sum(axis=1)
    S = segment_sums(x, max_len)
    score = np.full((T, max_len), np.inf)
    unit = np.full((T, max_len), -1, dtype=np.int32)
    gap = np.full((T, max_len), np.inf)
    B = np.zeros((T, max_len))
    for n in range(T):
        for l in range(1, min(max_len, n + 1) + 1):
            s = l * cn - 2.0 * (c64 @ S[n, l - 1])
            best, bk, second = np.inf, 0, np.inf
            for k in range(K):
                if s[k] < best:
                    best, bk, second = s[k], k, best
                elif s[k] < second:
                    second = s[k]
            score[n, l - 1], unit[n, l - 1] = best, bk
            gap[n, l - 1] = second - best if np.isfinite(best) else np.inf
            B[n, l - 1] = 2.0 ** -23 * (D + 2) * ((S[n, l - 1] ** 2).sum() / l + l * cn.max())
    return score, unit, gap, B


def scores(x, cent, max_len):
    """scores_loops with the loops over l and k as numpy expressions (the loop over the rows stays): the same sums in the same
    order -- numpy's cumsum adds one entry after the other -- so S64 has the same bits; the dots are a matrix product's, equal to
    the loops' to float64 rounding (tests/test_segment_cpu.py holds the two against each other).  What the GPU tests call on their larger cases."""
    x, cent = np.asarray(x, dtype=np.float32), np.asarray(cent, dtype=np.float32)
    T, D = x.shape
    K = cent.shape[0]
    c64, x64 = cent.astype(np.float64), x.astype(np.float64)
    cn = (c64 * c64).sum(axis=1)
    score = np.full((T, max_len), np.inf)
    unit = np.full((T, max_len), -1, dtype=np.int32)
    gap = np.full((T, max_len), np.inf)
    B = np.zeros((T, max_len))
    for n in range(T):
        m = min(max_len, n + 1)
        S = np.cumsum(x64[n - m + 1:n + 1][::-1], axis=0)  # (m, D): row l - 1 is S64(n, l)
        ls = np.arange(1, m + 1, dtype=np.float64)
        s = ls[:, None] * cn[None, :] - 2.0 * (S @ c64.T)
        s = np.where(np.isnan(s), np.inf, s)
        bk = s.argmin(axis=1)  # (the first of equal ones)
        best = s[np.arange(m), bk]
        score[n, :m], unit[n, :m] = best, bk
        if K > 1:
            second = np.partition(s, 1, axis=1)[:, 1]
            with np.errstate(invalid="ignore"):
                gap[n, :m] = np.where(np.isfinite(best), second - best, np.inf)
        B[n, :m] = 2.0 ** -23 * (D + 2) * ((S * S).sum(axis=1) / ls + ls * cn.max())
    return score, unit, gap, B


def batch_scores(x, cent, utt_ptr, max_len):
    """The rows of all utterances one after the other -> scores() of each, concatenated."""
    parts = [scores(np.asarray(x)[int(a):int(b)], cent, max_len) for a, b in zip(utt_ptr[:-1], utt_ptr[1:])]
    if not parts:
        parts = [scores(np.zeros((0, np.asarray(x).shape[1]), np.float32), cent, max_len)]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


# ---------------------------------------------------------------------------------------------------------------------- DP
def dp_alpha(score, lam):
    """-> (alpha (T + 1,) float64, back (T + 1,) int64) of the header's recursion on one utterance's (T, Lmax) scores: one rounding
    per addition, the smallest l of equal candidates, +inf and NaN never win (with nothing else: +inf and l = 1)."""
    score = np.asarray(score).astype(np.float64)  # (exact from f32)
    T, Lmax = score.shape
    lam = np.float64(lam)
    alpha = np.zeros(T + 1, dtype=np.float64)
    back = np.zeros(T + 1, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for t in range(1, T + 1):
            m = min(Lmax, t)
            v = alpha[t - m:t][::-1] + score[t - 1, :m]  # entry l - 1: alpha[t - l] + score[t - 1][l - 1]
            v = np.where(v < np.inf, v, np.inf)  # (NaN and +inf never win)
            bl = int(v.argmin())  # (the first of equal ones: the smallest l)
            alpha[t] = v[bl] + lam
            back[t] = bl + 1
    return alpha, back


def dp(score, unit, lam):
    """One utterance's (T, Lmax) scores (f32 or f64; taken to float64 exactly) and units ->
    (starts: the first frame of every segment, units: one per segment, cost = alpha[T], flag).  flag is NOT_FINITE (and starts,
    units empty, cost alpha[T]) when alpha[T] is not finite."""
    alpha, back = dp_alpha(score, lam)
    T = alpha.shape[0] - 1
    if not np.isfinite(alpha[T]):
        return np.zeros(0, np.int64), np.zeros(0, np.int32), alpha[T], NOT_FINITE
    starts, units = [], []
    t = T
    while t > 0:
        l = int(back[t])
        starts.append(t - l)
        units.append(int(unit[t - 1, l - 1]))
        t -= l
    return np.asarray(starts[::-1], dtype=np.int64), np.asarray(units[::-1], dtype=np.int32), alpha[T], 0


def frame_outputs(starts, units, T):
    """(starts, units) of one utterance -> (seg_unit (T,) int32, seg_start (T,) uint8): what fhvae_seg_dp writes per frame."""
    seg_unit, seg_start = np.zeros(T, dtype=np.int32), np.zeros(T, dtype=np.uint8)
    ends = list(starts[1:]) + [T]
    for a, b, k in zip(starts, ends, units):
        seg_unit[int(a):int(b)] = k
        seg_start[int(a)] = 1
    return seg_unit, seg_start


def objective(x, cent, starts, units, lam):
    """J64 of a segmentation of one utterance: sum over the segments of l |c_k|^2 - 2 S . c_k + lam, in float64 (|x|^2 dropped)."""
    x64, c64 = np.asarray(x, dtype=np.float64), np.asarray(cent, dtype=np.float64)
    T = x64.shape[0]
    ends = list(starts[1:]) + [T]
    total = 0.0
    for a, b, k in zip(starts, ends, units):
        S = x64[int(a):int(b)].sum(axis=0)
        total += (int(b) - int(a)) * float(c64[k] @ c64[k]) - 2.0 * float(S @ c64[k]) + float(lam)
    return total


def bound_of(B, starts, T):
    """The sum of B over the segments (starts) of an utterance of T frames."""
    ends = list(starts[1:]) + [T]
    return float(sum(B[int(b) - 1, int(b) - int(a) - 1] for a, b in zip(starts, ends)))


def brute_force(score, lam, max_len):
    """The minimum over all 2^(T-1) cuts of the sum of score[end - 1][l - 1] + lam over the segments, segments longer than
    max_len left out -> (J, starts); (inf, None) without a cut.  Of equal sums (exact on integer scores) the cut whose lengths,
    read from the LAST segment backwards, come first in lexicographic order: the recursion's "smallest l" at every step."""
    T = score.shape[0]
    if T == 0:
        return 0.0, []
    best, arg, key = np.inf, None, None
    for cuts in itertools.product((0, 1), repeat=T - 1):
        starts = [0] + [i + 1 for i, c in enumerate(cuts) if c]
        ends = starts[1:] + [T]
        if max(b - a for a, b in zip(starts, ends)) > max_len:
            continue
        j = math.fsum(float(score[b - 1, b - a - 1]) + float(lam) for a, b in zip(starts, ends))
        order = [b - a for a, b in zip(starts, ends)][::-1]
        if j < best or (j == best and order < key):
            best, arg, key = j, starts, order
    return best, arg


# ----------------------------------------------------------------------------------------------------------------- planted
def planted(rng, n_utt, K, D, max_len, noise=1e-3):
    """Utterances that are runs of 1 .. max_len frames of centroids at least 1 apart, consecutive runs of different units, with
    noise -> (x f32, cent f32, lengths, [(starts, units)] per utterance)."""
    cent = np.zeros((K, D), dtype=np.float32)
    for k in range(K):
        cent[k, k % D] = 1.0 + k // D
        cent[k, (k + 1) % D] = -0.5 * (k % 3)
    d = np.sqrt(((cent[:, None, :] - cent[None, :, :]) ** 2).sum(-1))
    assert K == 1 or d[~np.eye(K, dtype=bool)].min() >= 1.0
    rows, lengths, truth = [], [], []
    for _ in range(n_utt):
        n_runs = int(rng.integers(1, 6))
        starts, units, t, prev = [], [], 0, -1
        for _ in range(n_runs):
            k = int(rng.integers(K))
            if K > 1:
                while k == prev:
                    k = int(rng.integers(K))
            l = int(rng.integers(1, max_len + 1))
            starts.append(t)
            units.append(k)
            rows.append(np.repeat(cent[k][None], l, axis=0) + noise * rng.standard_normal((l, D)).astype(np.float32))
            t, prev = t + l, k
        lengths.append(t)
        truth.append((np.asarray(starts, np.int64), np.asarray(units, np.int32)))
    return np.concatenate(rows).astype(np.float32), cent, np.asarray(lengths, np.int64), truth


# ------------------------------------------------------------------------------------------------------------- boundaries
def boundary_scores(hyp, ref, tol):
    """hyp, ref: one sorted list of boundary times per utterance -> (hits, n_hyp, n_ref) by the two-pointer sweep: in time order,
    a pair within tol (to 1e-9) is a hit and uses both up; else the earlier of the two is dropped."""
    hits = nh = nr = 0
    for h, r in zip(hyp, ref):
        i = j = 0
        nh, nr = nh + len(h), nr + len(r)
        while i < len(h) and j < len(r):
            if abs(h[i] - r[j]) <= tol + 1e-9:
                hits, i, j = hits + 1, i + 1, j + 1
            elif h[i] < r[j]:
                i += 1
            else:
                j += 1
    return hits, nh, nr
