"""features.py -- log-mel (fbank) and log-magnitude (spec) features from PCM WAV files on the MI355X.

The reference computes them per file on the CPU with librosa 0.8.0 (prepare_numpy_data.generate_feat, :14-46, on
AudioUtils.stft / rstft / to_melspec, utils.py:155-272).  Here the arithmetic runs in one launch per batch of utterances
(fhvae_feats_fwd, csrc/feats.hip); this module holds the host side:

  read_wav            RIFF WAV, integer PCM (8-bit unsigned, 16, 24, 32-bit) -> float32 mono, scaled like soundfile
                      (int16 / 2**15, int24 / 2**23, int32 / 2**31, (u8 - 128) / 128); channels averaged.  No resampling.
  frame_sizes         n_fft = win_length = int(sr * win_t), hop = int(sr * hop_t) (the reference's truncation)
  dft_basis           windowed cos / -sin columns (periodic Hamming), built in float64, rounded to f32, padded for the kernel
  mel_filters         librosa.filters.mel(sr, n_fft', n_mels, fmin=0, fmax=sr/2, htk=False, norm='slaney') in float64, with
                      n_fft' = 2 * (n_bins - 1): melspectrogram(S=...) recovers n_fft from S's row count (odd n_fft differs)
  compute_features    a list of waveforms -> a list of (nframes, n_out) float32 arrays, batched into bounded launches

Utterances shorter than n_fft // 2 + 1 samples are an error (one reflection of the centre padding must suffice; numpy's
repeated reflection for shorter inputs is not reproduced).
"""
from __future__ import annotations

import wave as _wave

import numpy as np

FTYPES = ("fbank", "spec")
LOG_FLOOR = {"fbank": -20.0, "spec": -50.0}  # utils.py:233 / :199
MAX_NFFT = 2048  # FHVAE_FEATS_MAX_NFFT
MAX_NMELS = 256  # FHVAE_FEATS_MAX_NMELS
BATCH_SAMPLES = 1 << 24  # samples per launch (about 17 minutes at 16 kHz)


# ---------------------------------------------------------------------------------------------------------- audio input
def read_wav(path):
    """-> (samples float32 (n,), sample rate).  Integer PCM only; anything else raises ValueError naming the file."""
    try:
        with _wave.open(str(path), "rb") as w:
            nch, width, sr, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
            raw = w.readframes(n)
    except (_wave.Error, EOFError) as e:  # not RIFF, or a format the wave module does not read (float, extensible, ...)
        raise ValueError("%s: not a PCM WAV file (%s)" % (path, e)) from None
    if width not in (1, 2, 3, 4) or nch < 1:
        raise ValueError("%s: unsupported sample width %d bytes" % (path, width))
    n = len(raw) // (width * nch)
    b = np.frombuffer(raw, dtype=np.uint8, count=n * width * nch)
    if width == 1:
        x = (b.astype(np.float32) - 128.0) / 128.0
    elif width == 2:
        x = b.view("<i2").astype(np.float32) / 32768.0
    elif width == 3:
        t = b.reshape(-1, 3).astype(np.int32)
        v = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(np.float32) / float(1 << 23)
    else:
        x = b.view("<i4").astype(np.float32) / float(1 << 31)
    x = x.reshape(n, nch)
    y = x[:, 0] if nch == 1 else x.mean(axis=1, dtype=np.float32)
    return np.ascontiguousarray(y, dtype=np.float32), sr


# ---------------------------------------------------------------------------------------------------------- sizes, bases
def frame_sizes(sr, win_t=0.025, hop_t=0.010):
    """(n_fft, hop) by the reference's integer truncation (prepare_numpy_data.py:34, utils.py:182-183)."""
    return int(sr * win_t), int(sr * hop_t)


def num_frames(length, n_fft, hop):
    """Frames of a centred STFT of `length` samples: 1 + (length + 2 * (n_fft // 2) - n_fft) // hop."""
    return 1 + (length + 2 * (n_fft // 2) - n_fft) // hop


def hz_to_mel(f):
    """Slaney mel scale (librosa.hz_to_mel, htk=False): linear below 1 kHz, logarithmic above."""
    f = np.asarray(f, dtype=np.float64)
    lin = f / (200.0 / 3)
    log = 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0)
    return np.where(f >= 1000.0, log, lin)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    lin = m * (200.0 / 3)
    log = 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0))
    return np.where(m >= 15.0, log, lin)


def mel_filters(sr, n_fft, n_mels):
    """(n_mels, n_fft // 2 + 1) float64 slaney-normalised triangles, as librosa.filters.mel(sr, n_fft, n_mels) (0.8.0)."""
    fft_freqs = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2.0), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    weights = np.maximum(0.0, np.minimum(lower, upper))
    return weights * (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]


def _padded_sizes(n_fft):
    n_bins = n_fft // 2 + 1
    return (n_fft + 15) // 16 * 16, n_bins, (n_bins + 15) // 16


def dft_basis(n_fft):
    """The kernel's (32 * G, KP) f32 basis: row 32g + i = w[n] cos(2 pi n b / n_fft), row 32g + 16 + i = -w[n] sin(...), for
    bin b = 16g + i (zero rows past n_fft // 2, zero columns past n_fft); w = periodic Hamming (scipy get_window,
    fftbins=True).  Built in float64 with the phase reduced exactly (n * b mod n_fft), then rounded to f32."""
    KP, n_bins, G = _padded_sizes(n_fft)
    n = np.arange(n_fft)
    w = 0.54 - 0.46 * np.cos(2.0 * np.pi * n / n_fft)
    b = np.arange(n_bins)
    ph = 2.0 * np.pi * ((b[:, None] * n[None, :]) % n_fft) / n_fft
    out = np.zeros((G, 2, 16, KP), dtype=np.float64)
    c = np.zeros((16 * G, n_fft))
    s = np.zeros((16 * G, n_fft))
    c[:n_bins] = w * np.cos(ph)
    s[:n_bins] = -w * np.sin(ph)
    out[:, 0, :, :n_fft] = c.reshape(G, 16, n_fft)
    out[:, 1, :, :n_fft] = s.reshape(G, 16, n_fft)
    return out.reshape(32 * G, KP).astype(np.float32)


def mel_basis(sr, n_fft, n_mels):
    """The kernel's (16 * ceil(n_mels / 16), 16 * G) f32 mel basis for an STFT of n_fft points (n_fft' = 2 * (n_bins - 1))."""
    _, n_bins, G = _padded_sizes(n_fft)
    m = mel_filters(sr, 2 * (n_bins - 1), n_mels)
    out = np.zeros(((n_mels + 15) // 16 * 16, 16 * G), dtype=np.float32)
    out[:n_mels, :n_bins] = m
    return out


# ---------------------------------------------------------------------------------------------------------- the launch
def check_params(sr, ftype, win_t, hop_t, n_mels):
    if ftype not in FTYPES:
        raise ValueError("ftype must be one of %s, got %r" % (FTYPES, ftype))
    n_fft, hop = frame_sizes(sr, win_t, hop_t)
    if not 2 <= n_fft <= MAX_NFFT:
        raise ValueError("n_fft = int(sr * win_t) = %d is outside [2, %d]" % (n_fft, MAX_NFFT))
    if hop < 1:
        raise ValueError("hop = int(sr * hop_t) = %d must be at least 1" % hop)
    if ftype == "fbank" and not 1 <= n_mels <= MAX_NMELS:
        raise ValueError("n_mels = %d is outside [1, %d]" % (n_mels, MAX_NMELS))
    return n_fft, hop


class _Bases:
    """Device copies of the bases for one (sr, n_fft, n_mels, ftype), built once per compute_features call."""

    def __init__(self, sr, n_fft, n_mels, ftype, device):
        import torch

        self.dft = torch.from_numpy(dft_basis(n_fft)).to(device)
        self.mel = torch.from_numpy(mel_basis(sr, n_fft, n_mels)).to(device) if ftype == "fbank" else None


def _run_batch(hb, waves, n_fft, hop, n_mels, ftype, bases, device):
    import torch

    lens = np.array([len(w) for w in waves], dtype=np.int64)
    frames = num_frames(lens, n_fft, hop)
    wave_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    frame_ptr = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    n_out = n_mels if ftype == "fbank" else n_fft // 2 + 1
    host = torch.empty(int(wave_ptr[-1]), dtype=torch.float32, pin_memory=True)
    np.concatenate(waves, out=host.numpy())
    ptrs = torch.from_numpy(np.stack([wave_ptr, frame_ptr])).pin_memory()
    wave_d = host.to(device, non_blocking=True)
    ptrs_d = ptrs.to(device, non_blocking=True)
    out = torch.empty((int(frame_ptr[-1]), n_out), dtype=torch.float32, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    hb.feats_fwd(wave_d, ptrs_d[0], ptrs_d[1], bases.dft, bases.mel, n_fft, hop, n_mels, ftype, out, status)
    res = torch.empty(out.shape, dtype=torch.float32, pin_memory=True)
    res.copy_(out, non_blocking=True)
    st = status.cpu()  # (synchronises: the copy above is done too)
    if int(st.item()) != 0:
        raise RuntimeError("fhvae_feats_fwd: status %d (inconsistent wave_ptr / frame_ptr)" % int(st.item()))
    r = res.numpy()
    return [r[frame_ptr[j]:frame_ptr[j + 1]].copy() for j in range(len(waves))]


def batches(lengths, max_samples=BATCH_SAMPLES):
    """Consecutive index ranges [a, b) whose total length stays within max_samples (a longer utterance goes alone)."""
    out, a, tot = [], 0, 0
    for j, n in enumerate(lengths):
        if j > a and tot + n > max_samples:
            out.append((a, j))
            a, tot = j, 0
        tot += n
    if a < len(lengths):
        out.append((a, len(lengths)))
    return out


def compute_features(waves, sr, ftype="fbank", win_t=0.025, hop_t=0.010, n_mels=80, names=None, device="cuda",
                     max_samples=BATCH_SAMPLES):
    """Features of every waveform (float32 1-D arrays at rate `sr`) -> list of float32 (nframes, n_mels) for "fbank" or
    (nframes, n_fft // 2 + 1) for "spec", in input order.  Batched into launches of at most `max_samples` samples.
    `names` (optional) label the utterances in error messages."""
    import hip_binding as hb

    n_fft, hop = check_params(sr, ftype, win_t, hop_t, n_mels)
    waves = [np.ascontiguousarray(w, dtype=np.float32).reshape(-1) for w in waves]
    for j, w in enumerate(waves):
        if len(w) < n_fft // 2 + 1:
            name = names[j] if names is not None else "utterance %d" % j
            raise ValueError("%s: %d samples; at least n_fft // 2 + 1 = %d are needed" % (name, len(w), n_fft // 2 + 1))
    if not waves:
        return []
    bases = _Bases(sr, n_fft, n_mels, ftype, device)
    out = []
    for a, b in batches([len(w) for w in waves], max_samples):
        out.extend(_run_batch(hb, waves[a:b], n_fft, hop, n_mels, ftype, bases, device))
    return out
