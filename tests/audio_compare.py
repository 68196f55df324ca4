"""One comparator for the audio kernels (csrc/feats.hip, kaldi_fbank.hip, synth.hip, resample.hip), with bounds derived from
the arithmetic.  Every comparison is per element against a float64 oracle; no element is left out unless stated below.

The unit.  A kernel output starts as a dense product on the exact-f32 MFMA: a fixed-order f32 chain sum_k a_k b_k over
`terms` operand pairs (csrc/audio_tile.h: tile_product).  a_k are the gathered samples as the kernel holds them in LDS
(f32), b_k the f32 basis entries.  The unit of such an element is

    u = 2^-24 * sum_k |a_k| |b_k|                                   (test_resample_gpu, tests/head_elbo_compare.py)

Dense products (dense_bound, dense_units):  |got - want64| <= (terms + c) u + sum_k d_k |b_k|.
  terms   one rounding per accumulated product (the MFMA fuses multiply and add); padded columns hold exact zeros on one
          side, so they add nothing and `terms` is the logical chain length.
  c = 2   +1: the basis entries are float64 values rounded to f32 on the host (|b32 - b64| <= 2^-24 |b64|);
          +1: the second-order part of (1 + 2^-24)^(terms + 1) - 1 over terms <= 2048, and the f32 rounding of |a|, |b| in u.
  d_k     what the gather did to operand k before the chain, an absolute bound per operand (zero where the kernel loads
          f32 data as it is: synth_idft, synth_project, resample):
            feats:  a = fma(-0.97f, y[p-1], y[p]) -> d = 2^-24 |a| (the FMA's one rounding) + |0.97f - 0.97| |y[p-1]|
                    (0.97f is not 0.97; that part is in units of the previous sample, which |a| does not bound);
            kaldi:  mean = f32 sum / N in a fixed tree of depth D <= 3 ceil(N / 256) + 7, v = x - mean,
                    a = fma(-c, v[k-1], v[k]) -> dv = 2^-24 (D sum|x| / N + |v|), d = dv[k] + c dv[k-1] + 2^-24 |a|
                    + |c32 - c| |v[k-1]|.
        |a| in u is taken as |a64| + d, so u bounds the kernel's own operands.
  This is test_resample_gpu._units (c = 2, d = 0), moved here; that test calls dense_units.

Magnitudes (magnitude_bound):  m = sqrt(fma(c, c, s * s)).  The norm is 1-Lipschitz, so |m(c, s) - m64| <= hypot(Ec, Es);
  the product and the FMA round once each under the root (half of each survives it), the root rounds once, +1 for second
  order and a root within one ulp:  Em = hypot(Ec, Es) + 3 * 2^-24 (m64 + hypot(Ec, Es)).
  Power (kaldi):  p = fma(c, c, s * s):  Ep = (2 m64 + h) h + 2 * 2^-24 (m64 + h)^2, h = hypot(Ec, Es).

Mel products (mel_bound):  M_j = sum_b mag_b mel_jb, the same chain over n_bins terms with operand error Em:
  EM = sum_b mel32 Em + (n_bins + 2) 2^-24 sum_b mel32 (m64 + Em).

Logarithms (check_log):  out = max(logf(x), floor) with |x - want| <= E.
  want < e^floor           got must equal the floor exactly (silent frames, empty mel filters);
  want > 2 E               |got - max(log want, floor)| <= E / (want - E) + LOG_ULPS ulp of the result.  LOG_ULPS = 3: the
                           accuracy OpenCL requires of log and the device library's logf documents (its measured error
                           is below 1 ulp; the constant is the guarantee, not the measurement);
  else ("inside 2 E")      only got <= log(want + E) + the same ulps, or got == floor.  These are the excluded elements;
                           tests/test_audio_tiles_cpu.py asserts on the oracle alone that they are at most 1 % of a case.

synth_project's next = S a / (|a| + 1e-16) (direction_bound): where |a64| > 2 Ea the direction a / |a| moves by at most
  2 Ea / (|a64| - Ea) (either component), times S, plus 6 * 2^-24 S: the square, the FMA and the root (1.5 together), the
  added 1e-16 (one rounding, and itself below 2^-24 |a| wherever |a| > 2 Ea here), the division, the product, second order.
  With tprev, a = fma(-coef, tprev, rebuilt) adds 2^-24 |a| per component to Ea; coef is the f32 value on both sides.
  Where Ea = 0 and a64 = 0 (silent frames) next must be exactly 0; elsewhere inside 2 Ea only |next| <= S (1 + 6 * 2^-24).

synth_ola (ola_bound): the <= ceil(n_fft / hop) covering workspace elements are added in frame order (one rounding each),
  the f32 envelope likewise (n + 1 roundings: its entries are rounded squares), one division, one for second order:
  (sum of their bounds + (2 n + 4) 2^-24 sum |ws64|) / env64, n the count of covering frames.

The yardstick.  Besides the hard bound every case prints the worst and mean error in units (for logs: the linear error over
the propagated unit U, which is the bound with every count set to 1), for the kernel and for a float32 sequential emulation
of the oracle (emulate_*: one product after the other into an f32 accumulator, as resample_ref.resample_f32_sequential), and
asserts the kernel's figures within 2 x the emulation's (STAT in test_resample_gpu: the order differs, the chain lengths do
not).  The emulation's figures never come from a kernel's output.
  Kaldi's yardstick is taken on the mel energies before the logarithm (use-log-fbank=false, which the kernel offers; there
  the hard bound is E itself, on every element).  On the int16 scale log e is about 20, so one ulp of the logarithm is some
  20 * 2^-23 of e, several times the whole chain's error: measured on the logarithms the yardstick compared the device's
  logf (within 1 ulp) with numpy's (within half an ulp) and not the chains, and read 1.6 to 2.3 x at every height, the two
  that test_kaldi_fbank_gpu.py already covers included.  The logarithms keep their hard bound (LOG_ULPS).  feats has no
  linear output; there |log| is below 10 and the chains dominate.
"""
import numpy as np

EPS = 2.0 ** -24
LOG_ULPS = 3
STAT_FACTOR = 2.0
MAX_EXCLUDED = 0.01  # (tests/segment_cases.py, tests/test_units_gpu.py)


# ---------------------------------------------------------------------------------------------------------- dense products
def dense_bound(absA, absB, terms, c=2, dA=None):
    """absA (R, K) |a64|, absB (C, K) |b32|, dA (R, K) operand error -> (E, u), both (R, C)."""
    a = absA if dA is None else absA + dA
    u = EPS * (a @ absB.T)
    E = (terms + c) * u
    if dA is not None:
        E = E + dA @ absB.T
    return E, u


def dense_units(got, want, u, terms, c=2, extra=0.0, what="dense product"):
    """Asserts |got - want| <= (terms + c) u + extra per element; -> the errors in units of u where u > 0."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want)
    hard = (terms + c) * u + extra
    bad = err > hard
    assert not bad.any(), "%s: %d elements over the bound, worst |got - want| / bound = %g at %s" % (
        what, int(bad.sum()), (err[bad] / np.maximum(hard[bad], 1e-300)).max(), np.argwhere(bad)[0])
    m = u > 0
    return err[m] / u[m]


def magnitude_bound(c64, s64, Ec, Es):
    h = np.hypot(Ec, Es)
    return h + 3 * EPS * (np.hypot(c64, s64) + h)


def power_bound(c64, s64, Ec, Es):
    h, m = np.hypot(Ec, Es), np.hypot(c64, s64)
    return (2 * m + h) * h + 2 * EPS * (m + h) ** 2


def mel_bound(m64, Em, mel32, terms):
    """m64, Em (R, n_bins); mel32 (n_mels, n_bins) -> E (R, n_mels)."""
    a = np.abs(mel32).astype(np.float64)
    return Em @ a.T + (terms + 2) * EPS * ((m64 + Em) @ a.T)


# ---------------------------------------------------------------------------------------------------------- logarithms
def log_classes(want, E, floor):
    """-> (must_floor, compared, excluded) boolean masks over the elements of `want` (linear values)."""
    must_floor = want < np.exp(floor)
    compared = ~must_floor & (want > 2 * E)
    return must_floor, compared, ~must_floor & ~compared


def check_log(got, want, E, floor, what="log", enforce=True):
    """got f32 logs, want f64 linear oracle values, E their linear bound.  Asserts the rules of the module docstring;
    -> (compared mask, |exp(got) - want| on it).  enforce=False only measures (the float32 emulation: its pre-emphasis is no
    FMA, so the kernel's bound is not its bound)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.all(np.isfinite(got)), what
    g = got.astype(np.float64)
    fl = float(np.float32(floor))
    must_floor, compared, excluded = log_classes(want, E, floor)
    if not enforce:
        return compared, np.abs(np.exp(g[compared]) - want[compared])
    assert np.all(g[must_floor] == fl), "%s: %d elements below the floor are not the floor" % (what, int((g[must_floor] != fl).sum()))
    w = want[compared]
    lw = np.maximum(np.log(w), floor)
    slack = E[compared] / (w - E[compared])
    tol = slack + LOG_ULPS * 2 * EPS * (np.abs(lw) + slack)
    err = np.abs(g[compared] - lw)
    bad = err > tol
    assert not bad.any(), "%s: %d of %d elements over the bound, worst |dlog| / bound = %g (|dlog| %g)" % (
        what, int(bad.sum()), bad.size, (err[bad] / tol[bad]).max(), err[bad].max())
    with np.errstate(divide="ignore"):
        ceil = np.log(want[excluded] + E[excluded])
    ceil = ceil + LOG_ULPS * 2 * EPS * np.abs(ceil)
    ok = (g[excluded] <= np.maximum(ceil, fl)) | (g[excluded] == fl)
    assert ok.all(), "%s: %d elements inside 2 E exceed their ceiling" % (what, int((~ok).sum()))
    return compared, np.abs(np.exp(g[compared]) - w)


def direction_bound(a64, Ea, S):
    """|next - S a64 / |a64|| per component, where |a64| > 2 Ea (the mask is returned too)."""
    mag = np.abs(a64)
    ok = mag > 2 * Ea
    with np.errstate(divide="ignore", invalid="ignore"):
        b = S * (2 * Ea / (mag - Ea) + 6 * EPS)
    return np.where(ok, b, np.inf), ok


def ola_bound(Ews, absws, env64, count):
    """Sums over the covering frames already taken: Ews = sum of workspace bounds, absws = sum |ws64| -> bound per sample."""
    return (Ews + (2 * count + 4) * EPS * absws) / env64


# ---------------------------------------------------------------------------------------------------------- yardstick
def seq_f32(A32, B32):
    """(R, K) x (C, K) -> (R, C): one product after the other into an f32 accumulator, k ascending."""
    acc = np.zeros((A32.shape[0], B32.shape[0]), dtype=np.float32)
    for k in range(A32.shape[1]):
        acc += A32[:, k:k + 1] * B32[None, :, k]
    return acc


def stat_line(what, kernel_units, emu_units):
    """Prints the figures, asserts the kernel within STAT_FACTOR x the emulation's; -> the printed line."""
    k, e = (float(kernel_units.max()), float(kernel_units.mean())), (float(emu_units.max()), float(emu_units.mean()))
    line = "%-34s kernel max %7.3f mean %6.4f | f32 sequential max %7.3f mean %6.4f units" % (what, k[0], k[1], e[0], e[1])
    print(line)
    assert k[0] <= STAT_FACTOR * e[0] and k[1] <= STAT_FACTOR * e[1], line
    return line


# ---------------------------------------------------------------------------------------------------------- feats
def _reflect(x, pad):
    return np.pad(x, pad, mode="reflect") if pad else x


def hamming64(n_fft):
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def dft64(w, period, n_bins):
    """float64 (cos, -sin) rows (n_bins, len(w)) of the windowed DFT, the phase reduced exactly."""
    ph = 2.0 * np.pi * ((np.arange(n_bins)[:, None] * np.arange(len(w))[None, :]) % period) / period
    return w * np.cos(ph), -w * np.sin(ph)


def unpack_dft(basis32, n_bins, K):
    """The kernels' (32 G, KP) layout -> (cos, sin) f32 (n_bins, K)."""
    G = basis32.shape[0] // 32
    b = basis32.reshape(G, 2, 16, -1)
    return b[:, 0].reshape(16 * G, -1)[:n_bins, :K], b[:, 1].reshape(16 * G, -1)[:n_bins, :K]


def feats_frames(y, n_fft, hop, coef=0.97):
    """y f32 -> (A64, dA, Y, P): the pre-emphasised, reflected frames (F, n_fft) in float64, the gather's operand error, and the
    gathered y[p], y[p-1] the frames were made of."""
    y = np.asarray(y, dtype=np.float64)
    prev = np.concatenate([[0.0], y[:-1]])
    pad = n_fft // 2
    pre, yp, pp = _reflect(y - coef * prev, pad), _reflect(y, pad), _reflect(prev, pad)
    F = 1 + (len(y) + 2 * pad - n_fft) // hop
    idx = np.arange(F)[:, None] * hop + np.arange(n_fft)[None, :]
    A = pre[idx]
    return A, EPS * np.abs(A) + abs(float(np.float32(coef)) - coef) * np.abs(pp[idx]), yp[idx], pp[idx]


class FeatsOracle:
    """The float64 oracle of one utterance with its bounds.  lin: the linear value under the log, E its bound, U its unit."""

    def __init__(self, y, sr, n_fft, hop, n_mels, ftype, basis32, mel32=None, mel64=None):
        n_bins = n_fft // 2 + 1
        self.A, self.dA, self.Y, self.P = feats_frames(y, n_fft, hop)
        self.C64, self.S64 = dft64(hamming64(n_fft), n_fft, n_bins)
        self.C32, self.S32 = unpack_dft(basis32, n_bins, n_fft)
        self.mel32 = None if mel32 is None else np.asarray(mel32)[:n_mels, :n_bins]
        self.mel64, self.ftype, self.n_fft, self.n_bins = mel64, ftype, n_fft, n_bins
        self.floor = -20.0 if ftype == "fbank" else -50.0
        self.c, self.s = self.A @ self.C64.T, self.A @ self.S64.T
        self.lin = self.finish(self.c, self.s)
        absA = np.abs(self.A)
        Ec, uc = dense_bound(absA, np.abs(self.C32).astype(np.float64), n_fft, 2, self.dA)
        Es, us = dense_bound(absA, np.abs(self.S32).astype(np.float64), n_fft, 2, self.dA)
        m = np.hypot(self.c, self.s)
        self.E, self.U = magnitude_bound(self.c, self.s, Ec, Es), np.hypot(uc, us) + EPS * m
        if ftype == "fbank":
            self.E = mel_bound(m, self.E, self.mel32, n_bins)
            a = np.abs(self.mel32).astype(np.float64)
            self.U = self.U @ a.T + EPS * (m @ a.T)
        with np.errstate(divide="ignore"):
            self.U = self.U + EPS * np.abs(np.maximum(np.log(self.lin), self.floor)) * self.lin  # (the log's own rounding)
        self.silent = ~self.A.any(axis=1)

    def finish(self, c, s):
        m = np.hypot(c, s)
        return m @ self.mel64.T if self.ftype == "fbank" else m

    def emulate_f32(self):
        """The oracle's steps in sequential float32 -> f32 logs (F, n_out)."""
        f32 = np.float32
        A32 = self.Y.astype(f32) - f32(0.97) * self.P.astype(f32)  # (product and difference rounded: no FMA)
        c, s = seq_f32(A32, self.C32), seq_f32(A32, self.S32)
        m = np.sqrt(c * c + s * s)
        if self.ftype == "fbank":
            m = seq_f32(m, self.mel32)
        with np.errstate(divide="ignore"):
            return np.maximum(np.log(m), f32(self.floor)).astype(f32)

    def units(self, logs, enforce=True):
        """Checks f32 logs against the oracle (check_log) -> errors in units of U on the compared elements."""
        compared, err = check_log(logs, self.lin, self.E, self.floor, "%s n_fft %d" % (self.ftype, self.n_fft), enforce)
        assert not enforce or np.all(np.asarray(logs)[self.silent] == np.float32(self.floor))  # (silent frames: exactly the floor)
        return err / self.U[compared]

    def excluded_share(self):
        must_floor, compared, excluded = log_classes(self.lin, self.E, self.floor)
        return int(excluded.sum()), self.lin.size, must_floor


# ---------------------------------------------------------------------------------------------------------- synth
def synth_basis64(n_fft):
    """float64 (n_fft, 2 n_bins): row n . (re_0, im_0, re_1, ...) = window[n] * irfft(spectrum, n_fft)[n]."""
    n_bins = n_fft // 2 + 1
    c = np.full(n_bins, 2.0)
    c[0] = 1.0
    if n_fft % 2 == 0:
        c[-1] = 1.0
    ph = 2.0 * np.pi * ((np.arange(n_fft)[:, None] * np.arange(n_bins)[None, :]) % n_fft) / n_fft
    scale = hamming64(n_fft)[:, None] * c[None, :] / n_fft
    out = np.zeros((n_fft, 2 * n_bins))
    out[:, 0::2], out[:, 1::2] = scale * np.cos(ph), -scale * np.sin(ph)
    return out


def pack32(X):
    """complex (F, n_bins) -> what the device holds: f32 (F, n_bins, 2)."""
    return np.stack([X.real, X.imag], axis=-1).astype(np.float32)


def unpack64(P):
    P = np.asarray(P, dtype=np.float64)
    return P[..., 0] + 1j * P[..., 1]


def ola(rows, frames, n_fft, hop, dtype=np.float64):
    """rows (sum frames, n_fft) -> per utterance the plain overlap-add sums over the samples the device writes (the centre
    padding cut), frame after frame in `dtype`."""
    out, f0 = [], 0
    for F in frames:
        y = np.zeros(n_fft + hop * (F - 1), dtype=dtype)
        for f in range(F):
            y[f * hop:f * hop + n_fft] += rows[f0 + f]
        out.append(y[n_fft // 2:n_fft // 2 + hop * (F - 1)])
        f0 += F
    return np.concatenate(out)


class IstftOracle:
    """fhvae_synth_istft on spectrum X (complex with f32 parts) of utterances of `frames` frames: the workspace and the
    waveform in float64 with their bounds (E) and units (u), and the float32 sequential emulation of both."""

    def __init__(self, X, frames, n_fft, hop, basis32):
        F, n_bins = X.shape
        self.frames, self.n_fft, self.hop = list(frames), n_fft, hop
        self.A = pack32(X).reshape(F, 2 * n_bins).astype(np.float64)
        self.B32 = np.asarray(basis32)[:n_fft, :2 * n_bins]
        self.ws = self.A @ synth_basis64(n_fft).T
        self.terms = 2 * n_bins
        self.Ews, self.uws = dense_bound(np.abs(self.A), np.abs(self.B32).astype(np.float64), self.terms)
        w2 = hamming64(n_fft) ** 2
        one = np.ones((F, n_fft))
        env, cnt = ola(one * w2, frames, n_fft, hop), ola(one, frames, n_fft, hop)
        absws = ola(np.abs(self.ws), frames, n_fft, hop)
        self.y = ola(self.ws, frames, n_fft, hop) / env
        self.Ey = ola_bound(ola(self.Ews, frames, n_fft, hop), absws, env, cnt)
        self.uy = (ola(self.uws, frames, n_fft, hop) + EPS * absws) / env
        self.env32 = ola(one.astype(np.float32) * w2.astype(np.float32), frames, n_fft, hop, np.float32)

    def emulate_f32(self, utts):
        """The first `utts` utterances (the yardstick needs no more, and the loop is slow) -> (workspace rows, samples)."""
        rows = sum(self.frames[:utts])
        ws = seq_f32(self.A[:rows].astype(np.float32), self.B32)
        y = ola(ws, self.frames[:utts], self.n_fft, self.hop, np.float32)
        return ws, y / self.env32[:len(y)]


def stft_frames(y, frames, n_fft, hop):
    """Concatenated f32 waveforms of hop * (F - 1) samples -> (sum F, n_fft) float64 frames, numpy "reflect" padding of
    n_fft // 2 in front and n_fft - n_fft // 2 behind (synth_ref.stft), no pre-emphasis."""
    out, s0 = [], 0
    half = n_fft // 2
    for F in frames:
        L = hop * (F - 1)
        padded = np.pad(np.asarray(y[s0:s0 + L], dtype=np.float64), (half, n_fft - half), mode="reflect")
        out.append(padded[np.arange(F)[:, None] * hop + np.arange(n_fft)[None, :]])
        s0 += L
    return np.concatenate(out)


class ProjectOracle:
    """fhvae_synth_project: rebuilt = STFT(y), a = rebuilt - coef32 * tprev, next = S a / (|a| + 1e-16)."""

    def __init__(self, y32, frames, n_fft, hop, S, tprev, coef, basis32):
        n_bins = n_fft // 2 + 1
        self.A = stft_frames(y32, frames, n_fft, hop)
        C64, S64 = dft64(hamming64(n_fft), n_fft, n_bins)
        self.C32, self.S32 = unpack_dft(basis32, n_bins, n_fft)
        self.re, self.im = self.A @ C64.T, self.A @ S64.T
        absA = np.abs(self.A)
        self.Ere, self.ure = dense_bound(absA, np.abs(self.C32).astype(np.float64), n_fft)
        self.Eim, self.uim = dense_bound(absA, np.abs(self.S32).astype(np.float64), n_fft)
        self.terms, self.S = n_fft, np.asarray(S, dtype=np.float64)
        self.coef = float(np.float32(coef))
        self.tprev = None if tprev is None else unpack64(pack32(tprev))
        a = self.re + 1j * self.im
        Ea_re, Ea_im = self.Ere, self.Eim
        if self.tprev is not None:
            a = a - self.coef * self.tprev
            Ea_re, Ea_im = Ea_re + EPS * np.abs(a.real), Ea_im + EPS * np.abs(a.imag)
        self.a, self.Ea = a, np.hypot(Ea_re, Ea_im)
        self.next = self.S * a / (np.abs(a) + 1e-16)
        self.Enext, self.compared = direction_bound(a, self.Ea, self.S)
        self.zero = (self.S == 0) | ((self.Ea == 0) & (np.abs(a) == 0))  # S = 0 (silent frames) or a = 0 exactly: next is 0
        self.compared &= ~self.zero
        with np.errstate(divide="ignore", invalid="ignore"):
            self.unext = self.S * (2 * np.hypot(self.ure, self.uim) / np.abs(a) + EPS)

    def excluded(self):
        return int((~self.compared & ~self.zero).sum()), self.a.size

    def check(self, rebuilt, nxt, what):
        """rebuilt (or None), nxt: f32 (F, n_bins, 2) -> (units of rebuilt (re, im) (rows, n_bins, 2), units of next with NaN
        where it is not compared)."""
        ur = None
        if rebuilt is not None:
            dense_units(rebuilt[..., 0], self.re, self.ure, self.terms, what=what + " re")
            dense_units(rebuilt[..., 1], self.im, self.uim, self.terms, what=what + " im")
            ur = self.rebuilt_units(rebuilt)
        n = unpack64(nxt)
        assert np.all(np.isfinite(nxt)) and np.all(n[self.zero] == 0), what
        err = np.maximum(np.abs(n.real - self.next.real), np.abs(n.imag - self.next.imag))
        c = self.compared
        assert np.all(err[c] <= self.Enext[c]), "%s next: worst |err| / bound %g" % (what, (err[c] / self.Enext[c]).max())
        assert np.all(np.abs(n)[~c] <= self.S[~c] * (1 + 6 * EPS)), what
        return ur, self.next_units(nxt)

    def rebuilt_units(self, rebuilt):
        """|err| / u of the first len(rebuilt) rows, re and im, where u > 0."""
        r = len(rebuilt)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.stack([np.abs(rebuilt[..., 0] - self.re[:r]) / self.ure[:r], np.abs(rebuilt[..., 1] - self.im[:r]) / self.uim[:r]])
        return e[np.isfinite(e)]

    def next_units(self, nxt):
        r = len(nxt)
        n = unpack64(nxt)
        err = np.maximum(np.abs(n.real - self.next.real[:r]), np.abs(n.imag - self.next.imag[:r]))
        c = self.compared[:r]
        return err[c] / self.unext[:r][c]

    def emulate_f32(self, rows):
        """The first `rows` rows -> (rebuilt, next) f32 (rows, n_bins, 2)."""
        f32 = np.float32
        A32 = self.A[:rows].astype(f32)
        re, im = seq_f32(A32, self.C32), seq_f32(A32, self.S32)
        reb = np.stack([re, im], axis=-1)
        if self.tprev is not None:
            re, im = re - f32(self.coef) * self.tprev.real[:rows].astype(f32), im - f32(self.coef) * self.tprev.imag[:rows].astype(f32)
        sc = self.S[:rows].astype(f32) / (np.sqrt(re * re + im * im) + f32(1e-16))
        return reb, np.stack([re * sc, im * sc], axis=-1)


# ---------------------------------------------------------------------------------------------------------- kaldi fbank
class KaldiOracle(FeatsOracle):
    """Kaldi fbank (dither 0, remove-dc-offset, pre-emphasis c, povey window, power spectrum, log) of one utterance on the int16
    scale: the float64 oracle with its bounds, as FeatsOracle.  The floor is log(FLT_EPSILON), taken where e <= FLT_EPSILON."""

    def __init__(self, y, sr, N, S, P, n_mels, basis32, mel32, mel64, window64, coef=0.97):
        x = np.asarray(y, dtype=np.float64)
        F = 1 + (len(x) - N) // S
        self.X = x[np.arange(F)[:, None] * S + np.arange(N)[None, :]]
        mean = self.X.sum(axis=1, keepdims=True) / N
        v = self.X - mean
        vp = np.concatenate([v[:, :1], v[:, :-1]], axis=1)  # x[0] -= c x[0]
        self.A = v - coef * vp
        depth = 3 * -(-N // 256) + 7
        dv = EPS * (depth * np.abs(self.X).sum(axis=1, keepdims=True) / N + np.abs(v))
        dvp = np.concatenate([dv[:, :1], dv[:, :-1]], axis=1)
        self.c32 = np.float32(coef)
        self.dA = dv + coef * dvp + EPS * np.abs(self.A) + abs(float(self.c32) - coef) * np.abs(vp)
        n_bins = P // 2
        self.C64, self.S64 = dft64(window64, P, n_bins)
        self.C32, self.S32 = unpack_dft(basis32, n_bins, N)
        self.mel32, self.mel64 = np.asarray(mel32)[:n_mels, :n_bins], mel64
        self.ftype, self.n_fft, self.n_bins, self.floor = "kaldi", N, n_bins, float(np.log(2.0 ** -23))
        self.c, self.s = self.A @ self.C64.T, self.A @ self.S64.T
        self.lin = self.finish(self.c, self.s)
        absA = np.abs(self.A)
        Ec, uc = dense_bound(absA, np.abs(self.C32).astype(np.float64), N, 2, self.dA)
        Es, us = dense_bound(absA, np.abs(self.S32).astype(np.float64), N, 2, self.dA)
        p, m = self.c ** 2 + self.s ** 2, np.hypot(self.c, self.s)
        a = np.abs(self.mel32).astype(np.float64)
        self.E = mel_bound(p, power_bound(self.c, self.s, Ec, Es), self.mel32, n_bins)
        self.Ulin = (2 * m * np.hypot(uc, us) + EPS * p) @ a.T + EPS * (p @ a.T)
        with np.errstate(divide="ignore"):
            self.U = self.Ulin + EPS * np.abs(np.maximum(np.log(self.lin), self.floor)) * self.lin
        self.silent = ~self.X.any(axis=1)

    def units_linear(self, e, enforce=True):
        """The mel energies before the logarithm (use-log-fbank=false): |e - want| <= E on every element, no element left
        out -> the errors in units of the propagated unit, where that is positive."""
        e = np.asarray(e)
        assert e.dtype == np.float32 and e.shape == self.lin.shape
        err = np.abs(e.astype(np.float64) - self.lin)
        assert not enforce or np.all(err <= self.E), "kaldi N %d: worst |e - want| / bound %g" % (self.n_fft, (err / np.maximum(self.E, 1e-300)).max())
        m = self.Ulin > 0
        return err[m] / self.Ulin[m]

    def finish(self, c, s):
        return (c ** 2 + s ** 2) @ self.mel64.T

    def emulate_f32(self, log=True):
        f32 = np.float32
        X = self.X.astype(f32)
        mean = (np.cumsum(X, axis=1, dtype=f32)[:, -1:] / f32(self.n_fft)).astype(f32)
        v = X - mean
        A32 = v - self.c32 * np.concatenate([v[:, :1], v[:, :-1]], axis=1)
        c, s = seq_f32(A32, self.C32), seq_f32(A32, self.S32)
        e = seq_f32(c * c + s * s, self.mel32)
        if not log:
            return e
        with np.errstate(divide="ignore"):
            return np.where(e > f32(2.0 ** -23), np.log(e), f32(self.floor)).astype(f32)
