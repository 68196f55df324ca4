"""Float64 numpy oracle of the waveform synthesis (Griffin-Lim), written from the librosa 0.8.0 semantics of
griffinlim(S, n_iter, hop_length, win_length=n_fft, window="hamming", center=True, momentum, init=...) and its istft, and
independently of features.py.

  n_fft = int(sr * win_t), hop = int(sr * hop_t); periodic Hamming window; a spectrogram of F frames stands for
  hop * (F - 1) samples.
  istft: frame f is window * irfft(row f), added at f * hop; the sum is divided by the sum of the squared windows where that
         exceeds tiny(float32); n_fft // 2 samples are cut from the front and the output has hop * (F - 1) samples.
  stft:  F frames; padded = reflect(y, n_fft // 2 in front, n_fft - n_fft // 2 behind), so that frame F - 1 is complete
         for odd n_fft as well (even n_fft: librosa's symmetric centre padding); no pre-emphasis.
  griffinlim: angles <- initial unit phases, rebuilt <- 0; n_iter times { tprev <- rebuilt; y <- istft(S angles);
         rebuilt <- stft(y); a <- rebuilt - momentum / (1 + momentum) tprev; angles <- a / (|a| + 1e-16) }; y <- istft(S angles).

`dtype` (float64 by default) is the precision every stage is rounded to: float32 gives the emulation that the drift floor of
the GPU tests is measured with (numpy's FFT itself stays in double; its result is rounded).
"""
import math

import numpy as np


def sizes(sr, win_t=0.025, hop_t=0.010):
    return int(sr * win_t), int(sr * hop_t)


def window(n_fft):
    return np.array([0.54 - 0.46 * math.cos(2.0 * math.pi * n / n_fft) for n in range(n_fft)])


def istft(X, n_fft, hop, dtype=np.float64):
    """X (F, n_fft // 2 + 1) complex -> hop * (F - 1) samples."""
    X = np.asarray(X)
    F = X.shape[0]
    w = window(n_fft).astype(dtype)
    total = n_fft + hop * (F - 1)
    y = np.zeros(total, dtype=dtype)
    env = np.zeros(total, dtype=dtype)
    wsq = (w * w).astype(dtype)
    for f in range(F):
        seg = np.fft.irfft(X[f], n=n_fft).astype(dtype)
        y[f * hop:f * hop + n_fft] += w * seg
        env[f * hop:f * hop + n_fft] += wsq
    big = env > np.finfo(np.float32).tiny
    y[big] = y[big] / env[big]
    half = n_fft // 2
    return y[half:half + hop * (F - 1)].astype(dtype)


def stft(y, n_fft, hop, frames, dtype=np.float64):
    """-> (frames, n_fft // 2 + 1) complex."""
    cdtype = np.complex64 if dtype == np.float32 else np.complex128
    y = np.asarray(y, dtype=dtype)
    half = n_fft // 2
    padded = np.pad(y, (half, n_fft - half), mode="reflect")
    w = window(n_fft).astype(dtype)
    out = np.empty((frames, n_fft // 2 + 1), dtype=cdtype)
    for f in range(frames):
        out[f] = np.fft.rfft((w * padded[f * hop:f * hop + n_fft]).astype(dtype)).astype(cdtype)
    return out


def project(y, S, tprev, momentum, n_fft, hop, dtype=np.float64):
    """One round after the inverse: -> (rebuilt, S * angles)."""
    rebuilt = stft(y, n_fft, hop, S.shape[0], dtype)
    a = rebuilt if tprev is None else rebuilt - dtype(momentum / (1.0 + momentum)) * tprev
    angles = a / (np.abs(a) + dtype(1e-16))
    return rebuilt, (S.astype(dtype) * angles).astype(rebuilt.dtype)


def griffinlim(S, angles0, n_iter, momentum, n_fft, hop, dtype=np.float64, trace=None):
    """S (F, n_bins) magnitudes, angles0 (F, n_bins) complex unit phases -> hop * (F - 1) samples.  `trace` (a list)
    receives the waveform of every round."""
    cdtype = np.complex64 if dtype == np.float32 else np.complex128
    S = np.asarray(S, dtype=dtype)
    cur = (S * np.asarray(angles0)).astype(cdtype)
    tprev = None
    for _ in range(n_iter):
        y = istft(cur, n_fft, hop, dtype)
        if trace is not None:
            trace.append(y)
        rebuilt, cur = project(y, S, tprev, momentum, n_fft, hop, dtype)
        tprev = rebuilt
    y = istft(cur, n_fft, hop, dtype)
    if trace is not None:
        trace.append(y)
    return y


def spectral_convergence(y, S, n_fft, hop):
    """|| |stft(y)| - S ||_F / || S ||_F in float64."""
    S = np.asarray(S, dtype=np.float64)
    return float(np.linalg.norm(np.abs(stft(np.asarray(y, np.float64), n_fft, hop, S.shape[0])) - S) / np.linalg.norm(S))


def deemphasis(y, coef=0.97):
    """x[t] = y[t] + coef * x[t-1], serially in float64."""
    y = np.asarray(y, dtype=np.float64)
    x = np.empty_like(y)
    acc = 0.0
    for t in range(len(y)):
        acc = y[t] + coef * acc
        x[t] = acc
    return x


def unit_phases(seed, shape):
    """exp(2 pi i u), u uniform from RandomState(seed): the initial phases the tests hand to both sides."""
    u = np.random.RandomState(seed).rand(*shape)
    return np.exp(2j * np.pi * u)


def overlap_mean(segments, seg_len, seg_shift, nframes):
    """Mean over the segments (start k * seg_shift) covering each frame; frames past the last segment dropped."""
    nseg = len(segments)
    covered = min(nframes, (nseg - 1) * seg_shift + seg_len) if nseg else 0
    out = np.zeros((covered, segments.shape[2]), dtype=np.float64)
    cnt = np.zeros(covered)
    for k in range(nseg):
        a = k * seg_shift
        b = min(a + seg_len, covered)
        out[a:b] += segments[k, :b - a]
        cnt[a:b] += 1
    return out / cnt[:, None], covered


def speechlike(sr, n, seed):
    """Deterministic speech-like signal: gliding harmonic stack under three formant bumps, syllable-rate amplitude
    modulation, 1 % noise; n samples, peak about 0.5."""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / sr
    f0 = 110.0 + 40.0 * np.sin(2 * np.pi * 0.9 * t + seed)
    ph = 2 * np.pi * np.cumsum(f0) / sr
    y = np.zeros(n)
    formants = ((600.0, 150.0), (1400.0, 250.0), (2600.0, 350.0))
    for h in range(1, 40):
        fh = h * 130.0
        if fh >= 0.45 * sr:
            break
        gain = sum(math.exp(-0.5 * ((fh - c) / bw) ** 2) for c, bw in formants) + 0.02
        y += gain * np.sin(h * ph)
    y *= 0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t)
    y = 0.5 * y / max(np.abs(y).max(), 1e-9)
    return y + 0.005 * rng.standard_normal(n)
