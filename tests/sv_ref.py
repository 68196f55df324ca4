"""float64 oracle of the speaker-verification histogram (csrc/sv.hip) and of the equal error rate.

The f32 inputs are promoted to float64; scores, bins and per-edge counts are taken there.  An f32 score can fall on the other
side of a bin edge than its float64 value only when that value lies within DELTA of the edge:

    delta(D) = (2 D + 16) 2^-24

up to D 2^-24 from the f32 dot chain (|error| <= D u sum |a_k b_k| <= D u |a| |b|, u = 2^-24), the same from the two sums of
squares (a relative D u on each sum, halved by the square root, two of them), and 16 u for the square roots, the product of
the norms, the division and the bin arithmetic (one rounding each).  So for every edge k the kernel's count of trials in bins
>= k differs from the oracle's by at most the number of trials within delta of edge k.
"""
import numpy as np


def delta(D):
    return (2 * D + 16) * 2.0 ** -24


def make_case(S, D, speakers, seed):
    """centre[spk] + 0.7 randn, the speakers drawn uniformly -> (emb (S, D) f32, label (S,) int32)."""
    rs = np.random.RandomState(seed)
    centre = rs.randn(speakers, D)
    label = rs.randint(0, speakers, size=S).astype(np.int32)
    emb = (centre[label] + 0.7 * rs.randn(S, D)).astype(np.float32)
    return emb, label


def trial_scores(emb, label):
    """-> (target scores, non-target scores), float64, of the trials i < j with both labels >= 0."""
    e = np.asarray(emb, dtype=np.float32).astype(np.float64)
    label = np.asarray(label)
    n = np.maximum(np.sqrt((e * e).sum(axis=1)), 1e-30)
    score = (e @ e.T) / (n[:, None] * n[None, :])
    i, j = np.triu_indices(e.shape[0], k=1)
    ok = (label[i] >= 0) & (label[j] >= 0)
    i, j = i[ok], j[ok]
    same = label[i] == label[j]
    s = score[i, j]
    return s[same], s[~same]


def edge_counts(scores, NB, dlt):
    """For every edge k in 0..NB: (trials in bins >= k, trials within dlt of edge k).  Edge k sits at -1 + 2 k / NB; the
    clamp puts every trial in a bin >= 0 and none in a bin >= NB, so the two outer edges are exact."""
    s = np.sort(np.asarray(scores, dtype=np.float64))
    bins = np.clip(np.floor((s + 1.0) * (NB / 2)), 0, NB - 1).astype(np.int64)
    hist = np.bincount(bins, minlength=NB)
    cum = np.concatenate([np.cumsum(hist[::-1])[::-1], [0]])
    edges = -1.0 + 2.0 * np.arange(NB + 1) / NB
    near = np.searchsorted(s, edges + dlt, side="right") - np.searchsorted(s, edges - dlt, side="left")
    near[0] = near[NB] = 0
    return cum, near, hist


def near_share(scores, NB, dlt):
    """share of the trials within dlt of any inner edge"""
    s = np.asarray(scores, dtype=np.float64)
    pos = (s + 1.0) * (NB / 2)
    k = np.rint(pos)
    edge = -1.0 + 2.0 * k / NB
    inner = (k >= 1) & (k <= NB - 1)
    return float(np.mean(inner & (np.abs(s - edge) <= dlt))) if len(s) else 0.0


def hist_ref(emb, label, NB):
    tar, non = trial_scores(emb, label)
    return np.stack([edge_counts(tar, NB, 0.0)[2], edge_counts(non, NB, 0.0)[2]])


def exact_eer(tar, non):
    """The EER from the sorted float64 scores: thresholds at every distinct score (accept iff score >= threshold) and above
    the largest; where |FRR - FAR| is smallest, their mean."""
    tar, non = np.sort(tar), np.sort(non)
    th = np.unique(np.concatenate([tar, non]))
    frr = np.concatenate([np.searchsorted(tar, th, side="left"), [len(tar)]]) / len(tar)
    far = np.concatenate([len(non) - np.searchsorted(non, th, side="left"), [0]]) / len(non)
    k = int(np.argmin(np.abs(frr - far)))
    return 0.5 * (frr[k] + far[k])
