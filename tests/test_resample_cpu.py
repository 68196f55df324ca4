"""Resampling without a GPU: the kaiser_best filter table and the polyphase banks of features.py against the float64
oracle (tests/resample_ref.py), librosa's length rule, properties that do not depend on the reading of resampy (a sine
in the interior, a tone above the lower Nyquist rate), and the errors the host reports before any launch."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(44100, 16000), (22050, 16000), (48000, 16000), (8000, 16000), (16000, 22050), (11025, 16000)]
ALL_RATES = [8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000]


@pytest.fixture(scope="module")
def F():
    import features

    return features


def speechlike(sr, seconds, seed):
    """(the generator of test_feats_cpu.speechlike, copied)"""
    rng = np.random.default_rng(seed)
    t = np.arange(int(sr * seconds)) / sr
    f0 = 120 + 30 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f0) / sr
    y = sum(np.sin(h * ph) / h for h in range(1, 12)) * (0.5 + 0.4 * np.sin(2 * np.pi * 3 * t))
    y = 0.3 * y / np.abs(y).max() + 1e-3 * rng.standard_normal(len(t))
    return (np.round(y * 32767) / 32768).astype(np.float32)


def test_filter_table_matches_oracle(F):
    got, want = F.resample_filter(), R.filter_table()
    assert got.shape == want.shape == (32769,) and got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    big = np.abs(want) > 1e-6
    assert np.abs(got[big] / want[big] - 1).max() <= 1e-12
    assert got[0] == R.ROLLOFF == got.max()  # the peak; the full filter is this half mirrored about entry 0
    full = np.concatenate([got[:0:-1], got])
    assert np.array_equal(full, full[::-1]) and full.argmax() == len(got) - 1


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_bank_fir_matches_oracle(F, sr_in, sr_out):
    b = F.resample_bank(sr_in, sr_out)
    g = math.gcd(sr_in, sr_out)
    assert (b.L, b.M) == (sr_out // g, sr_in // g) and b.bank32.dtype == np.float32
    assert b.bank.shape == (b.NCP, b.KP) and b.NCP % 16 == 0 and b.KP % 16 == 0 and b.NCP >= b.P * b.L
    assert not b.bank[b.P * b.L:].any()
    # the chunk ranges cover every weight of their column group
    for gi, (c0, c1) in enumerate(b.chunks):
        blk = b.bank32[16 * gi:16 * gi + 16]
        assert not blk[:, :16 * c0].any() and not blk[:, 16 * c1:].any()
    long = speechlike(sr_in, 0.2, sr_in)
    half = len(b.alt) // 2
    for n in (3 * b.M, 3 * b.M + 1, 3 * b.M - 1, max(2, half // 3), len(long)):
        y = long[:n].astype(np.float64)
        assert len(y) == n
        want, _, _ = R.resample(y, sr_in, sr_out)
        got = F.resample_host(y, sr_in, sr_out)
        assert got.shape == want.shape
        err = np.abs(got - want).max() if len(want) else 0.0
        print("%d -> %d, n = %d: max |bank FIR - oracle| = %.3g of the signal's maximum" % (sr_in, sr_out, n, err / np.abs(y).max()))
        assert err <= 1e-10 * np.abs(y).max()


def test_time_register_exceptions_are_what_the_oracle_does(F):
    """Where the accumulated time register falls below an integer time, the oracle's n is one less than the exact one."""
    for sr_in, sr_out in PAIRS:
        b = F.resample_bank(sr_in, sr_out)
        periods = 40
        exc = b.exceptions(periods)
        time_register, inc, seen = 0.0, 1.0 / (float(sr_out) / sr_in), []
        for t in range(periods * b.L):
            if t % b.L == 0:
                seen.append(int(time_register) < (t // b.L) * b.M)
            time_register += inc
        if b.discontinuous:
            assert exc.tolist() == [int(s) for s in seen]
        else:
            assert not exc.any()
    assert F.resample_bank(44100, 16000).exceptions(4000).any()  # (so the alt weights are exercised)


def test_lengths(F):
    for sr_in, sr_out in PAIRS:
        ratio = float(sr_out) / sr_in
        M = sr_in // math.gcd(sr_in, sr_out)
        ns = list(range(0, 2001)) + [k * M for k in range(1, 60)] + [k * M + d for k in (7, 100, 1000) for d in (-1, 1)]
        for n in ns:
            assert F.resampled_length(n, sr_in, sr_out) == int(math.ceil(n * ratio)) == R.lengths(n, sr_in, sr_out)[1]
        arr = F.resampled_length(np.array(ns), sr_in, sr_out)
        assert arr.dtype == np.int64 and arr.tolist() == [int(math.ceil(n * ratio)) for n in ns]


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_sine_and_stopband(F, sr_in, sr_out):
    n = int(0.1 * sr_in)
    t_in, ratio = np.arange(n) / sr_in, float(sr_out) / sr_in
    got = F.resample_host(np.sin(2 * np.pi * 440.0 * t_in), sr_in, sr_out)
    t_out = np.arange(len(got)) / sr_out
    want = np.sin(2 * np.pi * 440.0 * t_out)
    edge = int(0.02 * sr_out)  # the filter's half width is at most 64 / min(rates) s = 8 ms
    err = np.abs(got - want)[edge:-edge].max()
    if ratio > 1:
        assert err <= 1e-6
    else:
        scale = ratio
        gain = scale * 512 / int(scale * 512)  # resampy's truncated index_step
        assert gain - 1 < 5e-3
        assert err <= (gain - 1) + 1e-6
    # a tone at 0.56 of the lower rate is above the lower Nyquist rate and below the higher one
    f = 0.56 * min(sr_in, sr_out)
    if f < 0.5 * sr_in:
        got = F.resample_host(np.sin(2 * np.pi * f * t_in), sr_in, sr_out)
        assert np.abs(got[edge:-edge]).max() < 1e-3
    else:  # upsampling: the tone cannot exist in the input; the image of a tone at 0.44 must be as low
        got = F.resample_host(np.sin(2 * np.pi * 0.44 * sr_in * t_in), sr_in, sr_out)
        spec = np.abs(np.fft.rfft(got[edge:-edge] * np.hanning(len(got) - 2 * edge)))
        freqs = np.fft.rfftfreq(len(got) - 2 * edge, 1.0 / sr_out)
        assert spec[freqs > 0.54 * sr_in].max() < 1e-3 * spec.max()


def test_every_common_pair_is_supported(F):
    for a in ALL_RATES:
        for b in ALL_RATES:
            if a != b:
                bank = F.resample_bank(a, b)
                assert 16 * (bank.KP + 4) <= F.RS_LDS_FLOATS and bank.NCP * bank.KP <= F.RS_MAX_BANK and bank.L <= F.RS_MAX_L


def test_host_errors(F, tmp_path):
    with pytest.raises(ValueError) as e:
        F.resample_bank(16000, 16001)
    assert "16000" in str(e.value) and "16001" in str(e.value) and str(F.RS_MAX_L) in str(e.value)
    with pytest.raises(ValueError) as e:  # few phases, but a window that 16 rows of LDS cannot hold
        F.resample_bank(48000, 1000)
    assert "48000" in str(e.value) and "1000" in str(e.value) and str(F.RS_LDS_FLOATS // 16 - 4) in str(e.value)
    with pytest.raises(ValueError):
        F.resample([np.zeros(10, np.float32)], 16000, 16001)
    same = [np.arange(5, dtype=np.float32)]
    assert F.resample(same, 16000, 16000)[0] is same[0]  # unchanged, as librosa
    with pytest.raises(ValueError, match="rates has 1 entries for 2"):
        F.compute_features([np.zeros(400, np.float32)] * 2, 16000, rates=[16000])
    with pytest.raises(ValueError, match="16001"):  # refused before anything is computed
        F.compute_features([np.zeros(400, np.float32)], 16000, rates=[16001])

    from test_feats_cpu import _write_wav

    d = tmp_path / "data" / "train"
    d.mkdir(parents=True)
    for j, sr in enumerate((16000, 8000)):
        _write_wav(d / ("u%d.wav" % j), np.zeros((4000, 1), np.int64), sr, 2)
    (d / "wav.scp").write_text("".join("u%d %s\n" % (j, d / ("u%d.wav" % j)) for j in range(2)))
    script = os.path.join(ROOT, "pytorch-scalablefhvae_amd", "prepare_numpy_data.py")
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, script, str(tmp_path / "data"), "--set_name", "train", "--resample"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "--resample needs --sr" in r.stderr, r.stderr
    r = subprocess.run([sys.executable, script, str(tmp_path / "data"), "--set_name", "train"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and not (d / "u0.npy").exists()
    assert "u1.wav: sample rate 8000 differs from 16000 (no resampling: convert the file or pass the matching --sr)" in r.stderr
    import prepare_numpy_data as P

    with pytest.raises(ValueError, match="--resample needs --sr"):
        P.prepare_numpy("librispeech", "train", str(tmp_path / "data"), resample=True)


def test_library_refuses_bad_arguments_before_any_launch(F):
    import ctypes

    import build_ext

    build_ext.build(verbose=False)
    import hip_binding as hb

    lib = hb.load_library()
    assert lib.fhvae_abi_version() == 12
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(n_in=100, U=1, n_rows=1, L=2, M=1, P=8, KP=256, WL=63, ratio=2.0, n_exc=0, alt_taps=0, alt_wl=0, n_out=200)

    def call(wave=p, bank=p, **kw):
        a = dict(ok, **kw)
        return lib.fhvae_resample_fwd(wave, a["n_in"], p, p, p, a["U"], a["n_rows"], bank, p, a["L"], a["M"], a["P"], a["KP"],
                                      a["WL"], a["ratio"], None, a["n_exc"], None, a["alt_taps"], a["alt_wl"], p, a["n_out"], p, None)

    assert call(wave=None) == -1 and call(bank=None) == -1
    assert call(U=0) == -2 and call(L=0) == -2 and call(KP=250) == -2 and call(ratio=0.0) == -2 and call(WL=-1) == -2
    assert call(L=F.RS_MAX_L + 1) == -5  # too many phases
    assert call(KP=2528) == -5  # 16 windows do not fit in LDS
    assert call(L=4096, P=4, KP=2048) == -5  # the bank is too large
    assert call(n_exc=5) == -1  # exceptions without their weights
    assert call(bank=ctypes.c_void_p(p.value + 4)) == -4
    assert lib.fhvae_resample_tile_rows(2528) == 0 and lib.fhvae_resample_tile_rows(100) == 0
    assert lib.fhvae_resample_tile_rows(2496) == 16 and lib.fhvae_resample_tile_rows(2512) == 0 and lib.fhvae_resample_tile_rows(624) == 32 and lib.fhvae_resample_tile_rows(800) == 32 and lib.fhvae_resample_tile_rows(256) == 64
    import torch

    t = torch.zeros(16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hb.resample_fwd(t, t, t, t, 1, t, t, 2, 1, 8, 63, 2.0, None, None, 0, t, t)
