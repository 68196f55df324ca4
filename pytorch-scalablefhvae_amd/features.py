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

and the way back for "spec" features (csrc/synth.hip: fhvae_synth_istft / _project / _deemph):

  synth_basis         window * irfft weights per output sample, (re, im) interleaved along the bins, float64 -> f32, padded
  window_sq           the squared window the overlap-add is normalised with
  synthesize          a list of (nframes, n_fft // 2 + 1) log-magnitude spectrograms -> a list of float32 waveforms by
                      Griffin-Lim (librosa 0.8.0 griffinlim semantics) and de-emphasis, batched into bounded launches
  write_wav           float32 mono -> 16-bit PCM WAV (the inverse of read_wav)

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
BATCH_FRAMES = 1 << 17  # frames per synthesis batch (about 22 minutes at a 10 ms hop; about 8 KB of device memory per frame)


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


# ---------------------------------------------------------------------------------------------------------- synthesis
def write_wav(path, y, sr):
    """Mono 16-bit PCM: samples clipped to [-1, 1) and scaled by 2**15 (read_wav gives them back within one step)."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(y)):
        raise ValueError("%s: the waveform has non-finite samples" % path)
    q = np.clip(np.round(y * 32768.0), -32768, 32767).astype("<i2")
    with _wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(sr))
        w.writeframes(q.tobytes())


def hamming(n_fft):
    """Periodic Hamming window (scipy get_window("hamming", n_fft, fftbins=True)) in float64."""
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def window_sq(n_fft):
    return (hamming(n_fft) ** 2).astype(np.float32)


def synth_basis(n_fft):
    """The kernel's (KP, K2P) f32 synthesis basis, KP = n_fft rounded up to 16, K2P = 2 * (n_fft // 2 + 1) rounded up to 16:
    row n . (re_0, im_0, re_1, im_1, ...) = window[n] * irfft(spectrum, n_fft)[n].  Column 2b holds
    w[n] c_b cos(2 pi b n / n_fft) / n_fft and column 2b + 1 holds -w[n] c_b sin(2 pi b n / n_fft) / n_fft, with c_b = 1 for
    bin 0 and (even n_fft) bin n_fft / 2 and 2 otherwise; the imaginary parts of those bins meet sin = 0, as irfft ignores
    them.  Built in float64 with the phase reduced exactly, then rounded to f32."""
    KP, n_bins, _ = _padded_sizes(n_fft)
    K2P = (2 * n_bins + 15) // 16 * 16
    n = np.arange(n_fft)
    b = np.arange(n_bins)
    c = np.full(n_bins, 2.0)
    c[0] = 1.0
    if n_fft % 2 == 0:
        c[-1] = 1.0
    ph = 2.0 * np.pi * ((n[:, None] * b[None, :]) % n_fft) / n_fft
    scale = hamming(n_fft)[:, None] * c[None, :] / n_fft
    out = np.zeros((KP, K2P), dtype=np.float64)
    out[:n_fft, 0:2 * n_bins:2] = scale * np.cos(ph)
    out[:n_fft, 1:2 * n_bins:2] = -scale * np.sin(ph)
    return out.astype(np.float32)


def check_synth_params(sr, win_t, hop_t, n_iter, momentum, preemphasis):
    n_fft, hop = check_params(sr, "spec", win_t, hop_t, 0)
    if hop > n_fft:
        raise ValueError("hop = %d exceeds n_fft = %d: the frames would leave gaps" % (hop, n_fft))
    if n_iter < 0:
        raise ValueError("n_iter = %d must not be negative" % n_iter)
    if not 0.0 <= momentum < 1.0:
        raise ValueError("momentum = %r is outside [0, 1)" % (momentum,))
    if not 0.0 <= preemphasis < 1.0:
        raise ValueError("preemphasis = %r is outside [0, 1)" % (preemphasis,))
    return n_fft, hop


def check_specs(specs, sr, n_fft, names=None):
    """-> the spectrograms as contiguous float32 arrays; ValueError for anything synthesize cannot invert."""
    n_bins = n_fft // 2 + 1
    out = []
    for j, S in enumerate(specs):
        name = names[j] if names is not None else "spectrogram %d" % j
        S = np.asarray(S)
        if S.ndim != 2:
            raise ValueError("%s: expected a (nframes, %d) array, got shape %s" % (name, n_bins, S.shape))
        if S.shape[1] != n_bins:
            hint = ""
            if S.shape[1] == 80:
                hint = " (80 columns look like ftype=\"fbank\" features: mel inversion is out of scope, only \"spec\" features can be synthesized)"
            raise ValueError("%s: %d columns, but sr %d and the window give n_fft // 2 + 1 = %d%s" % (name, S.shape[1], sr, n_bins, hint))
        if S.shape[0] < 2:
            raise ValueError("%s: %d frame(s); at least 2 are needed" % (name, S.shape[0]))
        out.append(np.ascontiguousarray(S, dtype=np.float32))
    return out


def frame_batches(frames, max_frames=BATCH_FRAMES):
    """Consecutive index ranges [a, b) whose total frame count stays within max_frames (a longer utterance goes alone)."""
    return batches(frames, max_frames)


class _SynthBases:
    def __init__(self, n_fft, device):
        import torch

        self.dft = torch.from_numpy(dft_basis(n_fft)).to(device)
        self.syn = torch.from_numpy(synth_basis(n_fft)).to(device)
        self.wsq = torch.from_numpy(window_sq(n_fft)).to(device)


def _synth_batch(hb, specs, phases, n_fft, hop, n_iter, momentum, preemphasis, log, bases, device):
    """Griffin-Lim of one batch; every round is two library calls on the stream, nothing is read back before the end."""
    import torch

    frames = np.array([len(S) for S in specs], dtype=np.int64)
    lens = hop * (frames - 1)
    wave_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    frame_ptr = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    n_frames, n_samples, n_bins = int(frame_ptr[-1]), int(wave_ptr[-1]), n_fft // 2 + 1
    ptrs_d = torch.from_numpy(np.stack([wave_ptr, frame_ptr])).to(device)
    mag = torch.from_numpy(np.concatenate(specs)).to(device)
    if log:
        mag = torch.exp(mag)
    ph = np.concatenate(phases)
    ang = torch.from_numpy(np.stack([ph.real, ph.imag], axis=-1).astype(np.float32)).to(device)
    cur = (mag.unsqueeze(-1) * ang).contiguous()
    del ang
    KP = (n_fft + 15) // 16 * 16
    ws = torch.empty((n_frames, KP), dtype=torch.float32, device=device)
    y = torch.empty(n_samples, dtype=torch.float32, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    coef = momentum / (1.0 + momentum)
    keep = [torch.empty_like(cur), torch.empty_like(cur)] if coef != 0.0 and n_iter > 1 else None
    tprev = None
    for it in range(n_iter):
        hb.synth_istft(cur, ptrs_d[0], ptrs_d[1], bases.syn, bases.wsq, n_fft, hop, ws, y, status)
        rebuilt = keep[it % 2] if keep is not None and it + 1 < n_iter else None  # (the last round's is never read)
        hb.synth_project(y, ptrs_d[0], ptrs_d[1], bases.dft, mag, tprev, coef, n_fft, hop, rebuilt, cur, status)
        tprev = rebuilt
    hb.synth_istft(cur, ptrs_d[0], ptrs_d[1], bases.syn, bases.wsq, n_fft, hop, ws, y, status)
    out = torch.empty_like(y)
    hb.synth_deemph(y, ptrs_d[0], preemphasis, out, status)
    res = torch.empty(out.shape, dtype=torch.float32, pin_memory=True)
    res.copy_(out, non_blocking=True)
    st = int(status.cpu().item())  # (synchronises: the copy above is done too)
    if st != 0:
        raise RuntimeError("fhvae_synth_*: status %d (inconsistent wave_ptr / frame_ptr)" % st)
    r = res.numpy()
    return [r[wave_ptr[j]:wave_ptr[j + 1]].copy() for j in range(len(specs))]


def synthesize(specs, sr, win_t=0.025, hop_t=0.010, n_iter=32, momentum=0.99, preemphasis=0.97, seed=0, init_phase=None,
               log=True, device="cuda", max_frames=BATCH_FRAMES, names=None):
    """Waveforms (float32, hop * (nframes - 1) samples each) of (nframes, n_fft // 2 + 1) spectrograms as
    compute_features(..., "spec") writes them (`log=True`: natural-log magnitudes; False: magnitudes), by n_iter rounds of
    Griffin-Lim with librosa 0.8.0's semantics and the inverse of the features' pre-emphasis (`preemphasis=0`: none).
    Initial phases are exp(2 pi i u), u drawn from numpy.random.RandomState(seed) utterance by utterance in input order,
    unless `init_phase` gives them: a list of complex (nframes, n_fft // 2 + 1) arrays of unit modulus.  Only "spec"
    features can be inverted; mel ("fbank") inversion is out of scope."""
    n_fft, hop = check_synth_params(sr, win_t, hop_t, n_iter, momentum, preemphasis)
    specs = check_specs(specs, sr, n_fft, names)
    if init_phase is not None:
        if len(init_phase) != len(specs):
            raise ValueError("init_phase has %d arrays for %d spectrograms" % (len(init_phase), len(specs)))
        init_phase = [np.asarray(p, dtype=np.complex128) for p in init_phase]
        for j, (p, S) in enumerate(zip(init_phase, specs)):
            if p.shape != S.shape:
                raise ValueError("init_phase[%d] has shape %s, the spectrogram %s" % (j, p.shape, S.shape))
    rng = np.random.RandomState(seed)
    if not specs:
        return []
    import hip_binding as hb

    bases = _SynthBases(n_fft, device)
    out = []
    for a, b in frame_batches([len(S) for S in specs], max_frames):
        phases = init_phase[a:b] if init_phase is not None else [np.exp(2j * np.pi * rng.rand(*S.shape)) for S in specs[a:b]]
        out.extend(_synth_batch(hb, specs[a:b], phases, n_fft, hop, n_iter, momentum, preemphasis, log, bases, device))
    return out
