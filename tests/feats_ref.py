"""Float64 numpy oracle of the feature extraction (log-mel "fbank" and log-magnitude "spec"), written from the librosa 0.8.0
semantics the reference relies on (prepare_numpy_data.py:14-46, utils.py:155-272) and independently of features.py.

  n_fft = int(sr * win_t), hop = int(sr * hop_t); pre-emphasis y[t] - 0.97 y[t-1]; centre padding n_fft // 2 in numpy
  "reflect" mode; periodic Hamming window; |rfft|; fbank: slaney mel filters for n_fft' = 2 * (n_bins - 1), log, floor -20;
  spec: log, floor -50.
"""
import math

import numpy as np


def sizes(sr, win_t=0.025, hop_t=0.010):
    return int(sr * win_t), int(sr * hop_t)


def n_frames(length, n_fft, hop):
    padded = length + 2 * (n_fft // 2)
    return 1 + (padded - n_fft) // hop


def slaney_hz_to_mel(f):
    if f < 1000.0:
        return f * 3.0 / 200.0
    return 15.0 + math.log(f / 1000.0) * 27.0 / math.log(6.4)


def slaney_mel_to_hz(m):
    if m < 15.0:
        return m * 200.0 / 3.0
    return 1000.0 * math.exp((m - 15.0) * math.log(6.4) / 27.0)


def mel_bank(sr, n_fft_eff, n_mels, bin_hz=None):
    """(n_mels, n_fft_eff // 2 + 1), one triangle at a time; bin k sits at k * sr / n_fft_eff Hz (or k * bin_hz)."""
    n_bins = n_fft_eff // 2 + 1
    step = (sr / 2.0) / (n_bins - 1) if bin_hz is None else bin_hz
    freqs = [k * step for k in range(n_bins)]
    top = slaney_hz_to_mel(sr / 2.0)
    pts = [slaney_mel_to_hz(top * j / (n_mels + 1)) for j in range(n_mels + 2)]
    bank = np.zeros((n_mels, n_bins))
    for i in range(n_mels):
        lo, mid, hi = pts[i], pts[i + 1], pts[i + 2]
        scale = 2.0 / (hi - lo)
        for k, f in enumerate(freqs):
            rise = (f - lo) / (mid - lo)
            fall = (hi - f) / (hi - mid)
            v = min(rise, fall)
            if v > 0.0:
                bank[i, k] = v * scale
    return bank


def spectrum(y, sr, win_t=0.025, hop_t=0.010):
    """|STFT| (nframes, n_fft // 2 + 1) in float64."""
    n_fft, hop = sizes(sr, win_t, hop_t)
    y = np.asarray(y, dtype=np.float64)
    pre = y.copy()
    pre[1:] = y[1:] - 0.97 * y[:-1]
    half = n_fft // 2
    padded = np.pad(pre, half, mode="reflect")
    window = np.array([0.54 - 0.46 * math.cos(2.0 * math.pi * n / n_fft) for n in range(n_fft)])
    nf = n_frames(len(y), n_fft, hop)
    out = np.empty((nf, n_fft // 2 + 1))
    for f in range(nf):
        seg = padded[f * hop:f * hop + n_fft]
        out[f] = np.abs(np.fft.rfft(window * seg))
    return out


def features(y, sr, ftype="fbank", win_t=0.025, hop_t=0.010, n_mels=80):
    """-> (nframes, n_mels) or (nframes, n_fft // 2 + 1) float64 (the floor applied; -inf never appears)."""
    S = spectrum(y, sr, win_t, hop_t)
    with np.errstate(divide="ignore"):
        if ftype == "spec":
            return np.maximum(np.log(S), -50.0)
        bank = mel_bank(sr, 2 * (S.shape[1] - 1), n_mels)
        return np.maximum(np.log(S @ bank.T), -20.0)
