"""Float64 numpy oracle of Kaldi's compute-fbank-feats (snip-edges framing), written from the description in
include/fhvae_hip.h and independently of features.py: plain loops, np.fft.rfft on the zero-padded frame, its own Philox4x32-10
and Box-Muller.  Also a float32 model of the same steps, which sets the error a float32 implementation may show."""
import math

import numpy as np

FLT_EPSILON = 2.0 ** -23
DEFAULTS = dict(sr=16000, frame_length=25.0, frame_shift=10.0, preemph=0.97, remove_dc=True, dither=0.0, window="povey",
                blackman_coeff=0.42, n_mels=23, low=20.0, high=0.0, use_log=True, use_power=True)


def sizes(sr, frame_length=25.0, frame_shift=10.0):
    N, S = int(sr * 0.001 * frame_length), int(sr * 0.001 * frame_shift)
    P = 1
    while P < N:
        P *= 2
    return N, S, P


def n_frames(n, N, S):
    return 0 if n < N else 1 + (n - N) // S


def window(N, kind, blackman_coeff=0.42):
    w = np.zeros(N)
    a = 2.0 * math.pi / (N - 1)
    for i in range(N):
        if kind == "hamming":
            w[i] = 0.54 - 0.46 * math.cos(a * i)
        elif kind == "hanning":
            w[i] = 0.5 - 0.5 * math.cos(a * i)
        elif kind == "povey":
            w[i] = (0.5 - 0.5 * math.cos(a * i)) ** 0.85
        elif kind == "rectangular":
            w[i] = 1.0
        elif kind == "blackman":
            w[i] = blackman_coeff - 0.5 * math.cos(a * i) + (0.5 - blackman_coeff) * math.cos(2 * a * i)
        else:
            raise ValueError(kind)
    return w


def mel(f):
    return 1127.0 * math.log(1.0 + f / 700.0)


def mel_bank(sr, P, n_mels, low=20.0, high=0.0):
    """(n_mels, P // 2) float64."""
    nyq = 0.5 * sr
    hi = high if high > 0 else nyq + high
    m_lo, m_hi = mel(low), mel(hi)
    delta = (m_hi - m_lo) / (n_mels + 1)
    bank = np.zeros((n_mels, P // 2))
    for b in range(n_mels):
        left, centre, right = m_lo + b * delta, m_lo + (b + 1) * delta, m_lo + (b + 2) * delta
        for i in range(P // 2):
            m = mel(i * sr / P)
            if left < m <= centre:
                bank[b, i] = (m - left) / (centre - left)
            elif centre < m < right:
                bank[b, i] = (right - m) / (right - centre)
    return bank


# ------------------------------------------------------------------------------------------------------------ dither noise
M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def uniform(r):
    return (2 * (r >> 9) + 1) * 2.0 ** -24


def frame_noise(seed, stream_id, frame, N):
    """Float64 standard normals of samples 0 .. N - 1 of frame `frame` (index within the utterance)."""
    g = np.zeros(4 * ((N + 3) // 4))
    key = (seed & M32, (seed >> 32) & M32)
    for q in range(len(g) // 4):
        r = philox4x32_10((frame & M32, q, stream_id & M32, (stream_id >> 32) & M32), key)
        for h in range(2):
            rad = math.sqrt(-2.0 * math.log(uniform(r[2 * h])))
            ang = 2.0 * math.pi * uniform(r[2 * h + 1])
            g[4 * q + 2 * h], g[4 * q + 2 * h + 1] = rad * math.cos(ang), rad * math.sin(ang)
    return g[:N]


def noise(seed, stream_id, frames, N):
    return np.stack([frame_noise(seed, stream_id, f, N) for f in range(frames)]) if frames else np.zeros((0, N))


# ------------------------------------------------------------------------------------------------------------ the features
def fbank(y, seed=0, stream_id=0, noise_in=None, **kw):
    """y: samples on the int16 scale.  -> float64 (frames, n_mels).  `noise_in` (frames, N) replaces the oracle's own noise."""
    o = dict(DEFAULTS, **kw)
    N, S, P = sizes(o["sr"], o["frame_length"], o["frame_shift"])
    y = np.asarray(y, dtype=np.float64)
    F = n_frames(len(y), N, S)
    w = window(N, o["window"], o["blackman_coeff"])
    bank = mel_bank(o["sr"], P, o["n_mels"], o["low"], o["high"])
    c = o["preemph"]
    out = np.zeros((F, o["n_mels"]))
    for f in range(F):
        x = y[f * S:f * S + N].copy()
        if o["dither"] != 0.0:
            x += o["dither"] * (noise_in[f] if noise_in is not None else frame_noise(seed, stream_id, f, N))
        if o["remove_dc"]:
            x -= x.sum() / N
        for i in range(N - 1, 0, -1):
            x[i] -= c * x[i - 1]
        x[0] -= c * x[0]
        x *= w
        spec = np.fft.rfft(np.concatenate([x, np.zeros(P - N)]))
        power = spec.real ** 2 + spec.imag ** 2
        if not o["use_power"]:
            power = np.sqrt(power)
        e = bank @ power[:P // 2]
        out[f] = np.log(np.maximum(e, FLT_EPSILON)) if o["use_log"] else e
    return out


def fbank_f32(y, noise_in=None, **kw):
    """The same steps with every operation rounded to float32 (numpy sums; a windowed DFT as a float32 matrix product):
    what any float32 implementation computes, up to summation order.  `noise_in` (frames, N) float32 when dither != 0."""
    o = dict(DEFAULTS, **kw)
    f32 = np.float32
    N, S, P = sizes(o["sr"], o["frame_length"], o["frame_shift"])
    y = np.asarray(y, dtype=f32)
    F = n_frames(len(y), N, S)
    w = window(N, o["window"], o["blackman_coeff"])
    n = np.arange(N)
    ph = 2.0 * np.pi * ((np.arange(P // 2)[:, None] * n[None, :]) % P) / P
    C, Sn = (w * np.cos(ph)).astype(f32), (-w * np.sin(ph)).astype(f32)
    bank = mel_bank(o["sr"], P, o["n_mels"], o["low"], o["high"]).astype(f32)
    c = f32(o["preemph"])
    out = np.zeros((F, o["n_mels"]), dtype=f32)
    for f in range(F):
        x = y[f * S:f * S + N].copy()
        if o["dither"] != 0.0:
            x = x + f32(o["dither"]) * np.asarray(noise_in[f], dtype=f32)
        if o["remove_dc"]:
            x = x - x.sum(dtype=f32) / f32(N)
        z = x.copy()
        z[1:] = x[1:] - c * x[:-1]
        z[0] = x[0] - c * x[0]
        re, im = C @ z, Sn @ z
        power = re * re + im * im
        if not o["use_power"]:
            power = np.sqrt(power)
        e = bank @ power
        out[f] = np.log(np.maximum(e, f32(FLT_EPSILON))) if o["use_log"] else e
    return out


def probe(sr=16000, seconds=2.0, seed=3):
    """The speech-like test signal: integer-valued, int16 scale, gated 140 Hz + 1330 Hz tones + noise, a DC offset of 700, a
    block of exact zeros (digital silence) and gaps of constant offset."""
    rng = np.random.default_rng(seed)
    n = int(sr * seconds)
    t = np.arange(n) / sr
    gate = (np.sin(2 * np.pi * 1.5 * t) > 0).astype(np.float64)
    y = gate * (3000.0 * np.sin(2 * np.pi * 140 * t) + 1200.0 * np.sin(2 * np.pi * 1330 * t) + 40.0 * rng.standard_normal(n))
    y = np.round(y) + 700.0
    y[int(0.2 * n):int(0.3 * n)] = 0.0
    return y
