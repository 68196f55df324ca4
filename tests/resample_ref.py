"""Float64 oracle of librosa 0.8.0's load-time resampling: librosa.resample(y, sr_in, sr_out, res_type="kaiser_best",
fix=True, scale=False) on resampy 0.2.2's resample_f, written from the published semantics and independently of
features.py (scipy supplies the Kaiser window here; features.py uses numpy.i0).

  filter_table()                      the half filter resampy ships as kaiser_best, rebuilt from its parameters
  resample(y, sr_in, sr_out)          -> (out float64 (ceil(n * ratio),), cond, taps): per output sample the conditioning
                                      c[t] = sum_j |h_j| |x_j| and the number of taps that met a sample of the utterance
  resample_f32_sequential(...)        float32 emulation of the reference's own arithmetic (numba adds one product after
                                      the other into a float32 output): the yardstick of the statistical bound

The sample loop keeps resampy's time register: it advances by repeated float64 addition of 1 / ratio, so at output
samples whose exact input time is an integer the register may sit just below it, and with it n and the filter phase
(resampy's truncated index_step makes the filter discontinuous there when downsampling).
"""
import math

import numpy as np
import scipy.signal

NUM_ZEROS = 64
PRECISION = 9
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
NUM_TABLE = 1 << PRECISION


def filter_table():
    n = NUM_TABLE * NUM_ZEROS
    taper = scipy.signal.get_window(("kaiser", BETA), 2 * n + 1, fftbins=False)[n:]
    return taper * ROLLOFF * np.sinc(ROLLOFF * np.linspace(0.0, NUM_ZEROS, n + 1))


def lengths(n_in, sr_in, sr_out):
    """(samples resampy computes, samples librosa returns)."""
    ratio = float(sr_out) / sr_in
    return int(n_in * ratio), int(math.ceil(n_in * ratio))


def _taps(table, delta, sr_in, sr_out, n_in):
    """Yields (t, sample indices, float64 weights) per computed output sample, in resampy's order (left wing, then right)."""
    ratio = float(sr_out) / sr_in
    scale = min(1.0, ratio)
    time_increment = 1.0 / ratio
    index_step = int(scale * NUM_TABLE)
    nwin = len(table)
    n_out = int(n_in * ratio)
    time_register = 0.0
    for t in range(n_out):
        n = int(time_register)
        frac = scale * (time_register - n)
        index_frac = frac * NUM_TABLE
        offset = int(index_frac)
        eta = index_frac - offset
        i_max = min(n + 1, (nwin - offset) // index_step)
        i = np.arange(i_max)
        wl = table[offset + i * index_step] + eta * delta[offset + i * index_step]
        frac = scale - frac
        index_frac = frac * NUM_TABLE
        offset = int(index_frac)
        eta = index_frac - offset
        k_max = min(n_in - n - 1, (nwin - offset) // index_step)
        k = np.arange(k_max)
        wr = table[offset + k * index_step] + eta * delta[offset + k * index_step]
        yield t, np.concatenate([n - i, n + 1 + k]), np.concatenate([wl, wr])
        time_register += time_increment


def _prepared(sr_in, sr_out):
    ratio = float(sr_out) / sr_in
    table = filter_table()
    if ratio < 1:
        table = table * ratio
    delta = np.zeros_like(table)
    delta[:-1] = np.diff(table)
    return table, delta


def resample(y, sr_in, sr_out):
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n_calc, n_ret = lengths(len(y), sr_in, sr_out)
    out, cond, taps = np.zeros(n_ret), np.zeros(n_ret), np.zeros(n_ret, dtype=np.int64)
    if sr_in == sr_out:
        return y.copy(), np.abs(y), np.ones(len(y), dtype=np.int64)
    table, delta = _prepared(sr_in, sr_out)
    ay = np.abs(y)
    for t, idx, w in _taps(table, delta, sr_in, sr_out, len(y)):
        out[t] = np.dot(w, y[idx])
        cond[t] = np.dot(np.abs(w), ay[idx])
        taps[t] = len(idx)
    return out, cond, taps


def resample_f32_sequential(y, sr_in, sr_out):
    """The reference's arithmetic: x float32, weights computed in float64 (table + eta * delta), each product
    weight * x[j] formed in float64 and added into the float32 output element, one tap after the other."""
    y = np.asarray(y, dtype=np.float32).reshape(-1)
    n_calc, n_ret = lengths(len(y), sr_in, sr_out)
    out = np.zeros(n_ret, dtype=np.float32)
    table, delta = _prepared(sr_in, sr_out)
    y64 = y.astype(np.float64)
    for t, idx, w in _taps(table, delta, sr_in, sr_out, len(y)):
        acc = np.float32(0.0)
        for p in w * y64[idx]:
            acc = np.float32(np.float64(acc) + p)
        out[t] = acc
    return out
