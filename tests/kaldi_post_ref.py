"""Float64 oracle of include/fhvae_kaldi_post.h: cepstra, delta features and sliding-window CMVN as plain numpy loops written
from the header (no Kaldi binary, no kernel code).  The log-mel rows in front of the cepstra come from kaldi_fbank_ref."""
import math

import numpy as np

import kaldi_fbank_ref as FB  # noqa: F401  (the log-mel oracle the end-to-end tests put in front)

CHUNK = 256  # FHVAE_KPOST_CHUNK


def dct64(C, B):
    m = np.zeros((C, B))
    for k in range(C):
        for j in range(B):
            m[k, j] = math.sqrt(1.0 / B) if k == 0 else math.sqrt(2.0 / B) * math.cos(math.pi / B * (j + 0.5) * k)
    return m


def lifter64(C, Q):
    return np.array([1.0 + 0.5 * Q * math.sin(math.pi * k / Q) for k in range(C)])


def cepstra(m, dct, lifter=None, energy=None, floor=-math.inf):
    """m (n, B), dct (C, B), lifter (C) as stored (float32 values) -> (float64 (n, C) exact result, float64 (n, C) the sum of
    |lifter_k dct_kj m_j| the error bound is stated in)."""
    m, dct = np.asarray(m, dtype=np.float64), np.asarray(dct, dtype=np.float64)
    lf = np.ones(len(dct)) if lifter is None else np.asarray(lifter, dtype=np.float64)
    out = (m @ dct.T) * lf[None, :]
    mag = (np.abs(m) @ np.abs(dct.T)) * np.abs(lf)[None, :]
    if energy is not None:
        out[:, 0] = np.maximum(np.asarray(energy, dtype=np.float64), floor)
        mag[:, 0] = 0.0
    return out, mag


def scales64(order, window):
    out = [np.ones(1)]
    norm = float(sum(j * j for j in range(-window, window + 1)))
    for _ in range(order):
        prev = out[-1]
        half = (len(prev) - 1) // 2
        cur = np.zeros(len(prev) + 2 * window)
        for j in range(-window, window + 1):
            for k in range(-half, half + 1):
                cur[j + k + half + window] += j * prev[k + half]
        out.append(cur / norm)
    return out


def add_deltas(x, scales):
    """One utterance x (T, D), scales as stored (float32 vectors) -> (float64 (T, (order + 1) D), the sum of |s_j x_j| of every
    element)."""
    x = np.asarray(x, dtype=np.float64)
    T, D = x.shape
    out, mag = np.zeros((T, len(scales) * D)), np.zeros((T, len(scales) * D))
    for i, s in enumerate(scales):
        s = np.asarray(s, dtype=np.float64)
        hw = (len(s) - 1) // 2
        for t in range(T):
            for m in range(len(s)):
                row = x[min(max(t + m - hw, 0), T - 1)]
                out[t, i * D:(i + 1) * D] += s[m] * row
                mag[t, i * D:(i + 1) * D] += np.abs(s[m] * row)
    return out, mag


def window(t, T, cmn_window, min_window, center):
    """The header's table, transcribed on its own (the test compares kaldi_post.cmvn_window with it)."""
    if center:
        b = t - cmn_window // 2
        e = b + cmn_window
    else:
        b = t - cmn_window
        e = t + 1
    if b < 0:
        e = e - b
        b = 0
    if not center:
        if e > t:
            e = max(t + 1, min_window)
    if e > T:
        b = b - (e - T)
        e = T
        if b < 0:
            b = 0
    return b, e


def _prefix(x):
    """S(t), t = 0 .. T, of one utterance's columns in the header's two-level order: float64 (T + 1, D)."""
    T, D = x.shape
    S = np.zeros((T + 1, D))
    P = np.zeros(D)
    for c0 in range(0, T + 1, CHUNK):
        q = np.zeros(D)
        for r in range(CHUNK):
            t = c0 + r
            if t > T:
                break
            S[t] = P + q
            if t < T:
                q = q + x[t]
        P = P + q  # (q: the chunk's total)
    return S


def cmvn_sliding(x, cmn_window, min_window, center, norm_vars):
    """One utterance x (T, D) float32 -> float32 (T, D), every operation the header's, in float64, rounded once at the end."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    T, D = x.shape
    S, S2 = _prefix(x), _prefix(x * x)
    out = np.zeros((T, D), dtype=np.float32)
    for t in range(T):
        b, e = window(t, T, cmn_window, min_window, center)
        N = float(e - b)
        mean = (S[e] - S[b]) / N
        y = x[t] - mean
        if norm_vars:
            var = np.maximum((S2[e] - S2[b]) / N - mean * mean, 1e-10)
            if e - b == 1:
                var = np.ones(D)
            y = y * (1.0 / np.sqrt(var))
        out[t] = y.astype(np.float32)
    return out
