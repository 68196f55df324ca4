"""Feature extraction without a GPU: the mel scale and basis against the float64 oracle (tests/feats_ref.py), the padded
kernel bases (a float32 numpy model of the kernel's products against the oracle), frame counts, the WAV reader, and the
argument errors that the host reports before any launch."""
import ctypes
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import feats_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def F():
    import features

    return features


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding as hb

    return hb.load_library()


def test_mel_scale_anchors(F):
    assert abs(float(F.hz_to_mel(1000.0)) - 15.0) < 1e-12
    assert abs(float(F.hz_to_mel(6400.0)) - 42.0) < 1e-9
    f = np.array([0.0, 50.0, 999.0, 1000.0, 1001.0, 4000.0, 6400.0, 11025.0])
    np.testing.assert_allclose(F.mel_to_hz(F.hz_to_mel(f)), f, rtol=1e-9, atol=1e-9)
    for x in f:
        assert abs(R.slaney_hz_to_mel(x) - float(F.hz_to_mel(x))) < 1e-9


@pytest.mark.parametrize("sr,n_fft,n_mels", [(16000, 400, 80), (8000, 200, 40), (22050, 551, 80)])
def test_mel_basis_matches_oracle(F, sr, n_fft, n_mels):
    n_bins = n_fft // 2 + 1
    want = R.mel_bank(sr, 2 * (n_bins - 1), n_mels)
    got = F.mel_filters(sr, 2 * (n_bins - 1), n_mels)
    assert got.shape == want.shape == (n_mels, n_bins)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6 * want.max())
    padded = F.mel_basis(sr, n_fft, n_mels)
    assert padded.shape == ((n_mels + 15) // 16 * 16, (n_bins + 15) // 16 * 16) and padded.dtype == np.float32
    np.testing.assert_allclose(padded[:n_mels, :n_bins], want, rtol=1e-6, atol=1e-6 * want.max())
    assert not padded[n_mels:].any() and not padded[:, n_bins:].any()
    if n_fft % 2:  # odd n_fft: the bins sit on n_fft' = n_fft - 1's grid (550 at 22.05 kHz), not at k * sr / n_fft
        other = R.mel_bank(sr, n_fft, n_mels, bin_hz=sr / n_fft)
        assert other.shape == want.shape and np.allclose(R.mel_bank(sr, n_fft - 1, n_mels), want)
        assert np.abs(padded[:n_mels, :n_bins] - other).max() > 1e-3 * want.max()


def test_frame_counts(F):
    for sr in (16000, 8000, 22050):
        n_fft, hop = F.frame_sizes(sr)
        assert (n_fft, hop) == R.sizes(sr)
        for L in (n_fft // 2 + 1, hop - 1, hop, hop + 1, 12345):
            want = len(np.pad(np.zeros(L), n_fft // 2, mode="reflect"))
            want = 1 + (want - n_fft) // hop
            assert F.num_frames(L, n_fft, hop) == R.n_frames(L, n_fft, hop) == want
    assert F.frame_sizes(22050) == (551, 220) and F.frame_sizes(16000) == (400, 160) and F.frame_sizes(8000) == (200, 80)
    # the explicit lengths of the issue at 16 kHz (n_fft 400, hop 160): 201, 159, 160, 161
    assert [F.num_frames(L, 400, 160) for L in (201, 159, 160, 161, 16000)] == [2, 1, 2, 2, 101]


def _model_f32(F, y, sr, ftype, n_mels=80):
    """The kernel's computation in float32 numpy: gathered frames . padded basis, |.|, . mel basis, log, floor."""
    n_fft, hop = F.frame_sizes(sr)
    y = np.asarray(y, np.float32)
    pre = y.copy()
    pre[1:] = y[1:] - np.float32(0.97) * y[:-1]
    padded = np.pad(pre, n_fft // 2, mode="reflect")
    nf = F.num_frames(len(y), n_fft, hop)
    B = F.dft_basis(n_fft)
    KP = B.shape[1]
    fr = np.zeros((nf, KP), np.float32)
    for f in range(nf):
        fr[f, :n_fft] = padded[f * hop:f * hop + n_fft]
    P = fr @ B.T  # (nf, 32G): per group, 16 cos columns then 16 sin columns
    G = B.shape[0] // 32
    P = P.reshape(nf, G, 2, 16)
    mag = np.sqrt(P[:, :, 0] ** 2 + P[:, :, 1] ** 2).reshape(nf, 16 * G)
    with np.errstate(divide="ignore"):
        if ftype == "spec":
            return np.maximum(np.log(mag[:, :n_fft // 2 + 1]), -50.0)
        M = mag @ F.mel_basis(sr, n_fft, n_mels).T
        return np.maximum(np.log(M[:, :n_mels]), -20.0)


def speechlike(sr, seconds, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(int(sr * seconds)) / sr
    f0 = 120 + 30 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f0) / sr
    y = sum(np.sin(h * ph) / h for h in range(1, 12)) * (0.5 + 0.4 * np.sin(2 * np.pi * 3 * t))
    y = 0.3 * y / np.abs(y).max() + 1e-3 * rng.standard_normal(len(t))
    return (np.round(y * 32767) / 32768).astype(np.float32)


@pytest.mark.parametrize("sr", [16000, 22050])
@pytest.mark.parametrize("ftype", ["fbank", "spec"])
def test_padded_bases_model_matches_oracle(F, sr, ftype):
    y = speechlike(sr, 0.4, sr)
    y[2000:4000] = 0.0
    got = _model_f32(F, y, sr, ftype)
    want = R.features(y, sr, ftype)
    assert got.shape == want.shape
    ok = np.abs(got - want) <= 5e-4
    fmax = np.exp(want).max(axis=1, keepdims=True)
    ok |= np.abs(np.exp(got) - np.exp(want)) <= 1e-6 * fmax
    assert ok.all(), np.abs(got - want).max()


def _write_wav(path, data, sr, width):
    """data: (n, ch) integer samples already in the file's range."""
    n, ch = data.shape
    if width == 1:
        raw = data.astype(np.uint8).tobytes()
    elif width == 2:
        raw = data.astype("<i2").tobytes()
    elif width == 3:
        v = data.astype(np.int64).reshape(-1) & 0xFFFFFF
        raw = np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()
    else:
        raw = data.astype("<i4").tobytes()
    with wave.open(str(path), "wb") as w:
        w.setnchannels(ch)
        w.setsampwidth(width)
        w.setframerate(sr)
        w.writeframes(raw)


@pytest.mark.parametrize("width", [1, 2, 3, 4])
@pytest.mark.parametrize("channels", [1, 2])
def test_wav_reader_round_trip(F, tmp_path, width, channels):
    rng = np.random.default_rng(width * 10 + channels)
    n = 1000
    if width == 1:
        data = rng.integers(0, 256, size=(n, channels))
        want = (data.astype(np.float64) - 128) / 128
    else:
        bits = 8 * width
        data = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=(n, channels), dtype=np.int64)
        data[0] = -(1 << (bits - 1))
        data[1] = (1 << (bits - 1)) - 1
        want = data.astype(np.float64) / (1 << (bits - 1))
    p = tmp_path / "x.wav"
    _write_wav(p, data, 11025, width)
    y, sr = F.read_wav(p)
    assert sr == 11025 and y.dtype == np.float32 and y.shape == (n,)
    want = want.astype(np.float32).mean(axis=1, dtype=np.float32) if channels > 1 else want[:, 0].astype(np.float32)
    np.testing.assert_allclose(y, want, rtol=0, atol=1e-7)
    if channels == 1:
        assert np.array_equal(y, want)


def test_wav_reader_rejects_other_formats(F, tmp_path):
    p = tmp_path / "float.wav"
    data = np.zeros(100, np.float32).tobytes()
    fmt = (b"fmt " + (16).to_bytes(4, "little") + (3).to_bytes(2, "little") + (1).to_bytes(2, "little") +
           (16000).to_bytes(4, "little") + (64000).to_bytes(4, "little") + (4).to_bytes(2, "little") + (32).to_bytes(2, "little"))
    body = b"WAVE" + fmt + b"data" + len(data).to_bytes(4, "little") + data
    p.write_bytes(b"RIFF" + len(body).to_bytes(4, "little") + body)
    with pytest.raises(ValueError, match="float.wav"):
        F.read_wav(p)
    q = tmp_path / "noise.flac"
    q.write_bytes(b"fLaC" + bytes(100))
    with pytest.raises(ValueError, match="noise.flac"):
        F.read_wav(q)


def test_feats_argument_errors_before_launch(lib, F):
    import hip_binding as hb

    assert hb.SIGNATURES["fhvae_feats_fwd"] and hb.SIGNATURES["fhvae_feats_tile_rows"]
    buf = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16  # a 16-byte aligned host address: never dereferenced here
    ok = dict(wave=p, n_samples=1000, wave_ptr=p, frame_ptr=p, U=1, n_frames=7, dft=p, mel=p, n_fft=400, hop=160, n_mels=80,
              ftype=0, out=p, status=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.fhvae_feats_fwd(a["wave"], a["n_samples"], a["wave_ptr"], a["frame_ptr"], a["U"], a["n_frames"], a["dft"],
                                   a["mel"], a["n_fft"], a["hop"], a["n_mels"], a["ftype"], a["out"], a["status"], None)

    for name in ("wave", "wave_ptr", "frame_ptr", "dft", "out", "status"):
        assert call(**{name: None}) == -1, name
    assert call(mel=None) == -1                      # fbank needs the mel basis
    assert call(n_fft=2049) == -5 and call(n_fft=1) == -5
    assert call(n_fft=1680) == -5                    # fbank tile beyond LDS (FHVAE_FEATS_MAX_NFFT_FBANK = 1664)
    assert call(n_mels=257) == -5 and call(n_mels=0) == -5
    assert call(hop=0) == -2 and call(U=0) == -2 and call(n_frames=0) == -2
    assert call(ftype=7) == -3
    assert call(dft=p + 4) == -4
    assert lib.fhvae_feats_tile_rows(400, 0) == 64 and lib.fhvae_feats_tile_rows(2048, 1) == 16
    assert lib.fhvae_feats_tile_rows(1664, 0) == 16 and lib.fhvae_feats_tile_rows(1665, 0) == 0
    assert lib.fhvae_feats_tile_rows(2049, 1) == 0 and lib.fhvae_feats_tile_rows(551, 0) > 0


def test_python_argument_errors(F):
    with pytest.raises(ValueError, match="utt_short"):
        F.compute_features([np.zeros(1000, np.float32), np.zeros(200, np.float32)], 16000, names=["ok", "utt_short"])
    with pytest.raises(ValueError, match="n_fft"):
        F.compute_features([np.zeros(100000, np.float32)], 16000, win_t=0.2)
    with pytest.raises(ValueError, match="n_mels"):
        F.compute_features([np.zeros(1000, np.float32)], 16000, n_mels=300)
    with pytest.raises(ValueError, match="ftype"):
        F.compute_features([np.zeros(1000, np.float32)], 16000, ftype="mfcc")
    assert F.batches([5, 5, 5, 20, 1], 10) == [(0, 2), (2, 3), (3, 4), (4, 5)]


def test_cli_rejects_other_sample_rate(F, tmp_path):
    d = tmp_path / "data" / "train"
    d.mkdir(parents=True)
    for j, sr in enumerate((16000, 8000)):
        _write_wav(d / ("u%d.wav" % j), np.zeros((4000, 1), np.int64), sr, 2)
    (d / "wav.scp").write_text("".join("u%d %s\n" % (j, d / ("u%d.wav" % j)) for j in range(2)))
    script = os.path.join(ROOT, "pytorch-scalablefhvae_amd", "prepare_numpy_data.py")
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    # --sr against the first file's rate, then (no --sr) the second file against the first
    for extra, bad in ((["--sr", "22050"], "u0.wav"), ([], "u1.wav")):
        r = subprocess.run([sys.executable, script, str(tmp_path / "data"), "--set_name", "train"] + extra,
                           capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode != 0 and "sample rate" in r.stderr and bad in r.stderr, r.stderr
        assert not (d / "u0.npy").exists()
