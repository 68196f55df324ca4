"""Kaldi data format without a GPU: the config parser, the mel bank and DFT basis against the float64 oracle
(tests/kaldi_fbank_ref.py), the oracle's own sanity, the ark / scp container byte for byte, KaldiDataset against NumpyDataset,
and the argument errors the library reports before any launch."""
import ctypes
import os
import struct

import numpy as np
import pytest

import kaldi_fbank_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "tests", "golden", "kaldi_fbank.conf")
FLOOR = float(np.log(2.0 ** -23))


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


# ------------------------------------------------------------------------------------------------------------ config parser
def test_config_parser_reference_settings(F):
    o = F.kaldi_fbank_options(CONF)
    assert set(o) == set(F.KALDI_DEFAULTS)
    assert o["window-type"] == "hamming" and o["use-energy"] is False and o["sample-frequency"] == 16000
    assert o["dither"] == 1.0 and o["num-mel-bins"] == 80 and o["htk-compat"] is True
    rest = {k: v for k, v in o.items() if k not in ("window-type", "use-energy", "sample-frequency", "dither", "num-mel-bins", "htk-compat")}
    assert rest == {"frame-length": 25.0, "frame-shift": 10.0, "preemphasis-coefficient": 0.97, "remove-dc-offset": True,
                    "blackman-coeff": 0.42, "low-freq": 20.0, "high-freq": 0.0, "use-log-fbank": True, "use-power": True,
                    "snip-edges": True, "round-to-power-of-two": True, "energy-floor": 0.0, "raw-energy": True}
    d = F.kaldi_fbank_options(None)
    assert d["window-type"] == "povey" and d["num-mel-bins"] == 23 and d["dither"] == 1.0
    assert F.kaldi_fbank_options({"num-mel-bins": 40, "dither": 0})["num-mel-bins"] == 40
    assert F.kaldi_fbank_options(o) == o
    assert F.kaldi_frame_sizes(o) == (400, 160, 512) == R.sizes(16000)
    assert F.kaldi_frame_sizes(F.kaldi_fbank_options({"sample-frequency": 8000})) == (200, 80, 256) == R.sizes(8000)


@pytest.mark.parametrize("line,word", [("--no-such-option=1", "no-such-option"), ("--use-energy=true", "use-energy"),
                                       ("--snip-edges=false", "snip-edges"), ("--vtln-low=100", "vtln-low"),
                                       ("--round-to-power-of-two=false", "round-to-power-of-two"),
                                       ("--window-type=triangle", "window-type"), ("--num-mel-bins=many", "num-mel-bins"),
                                       ("num-mel-bins=3", "num-mel-bins")])
def test_config_parser_refuses(F, tmp_path, line, word):
    p = tmp_path / "bad.conf"
    p.write_text("# a comment\n\n--dither=0  # trailing comment\n%s\n" % line)
    with pytest.raises(ValueError, match=word) as e:
        F.kaldi_fbank_options(p)
    assert "bad.conf" in str(e.value)
    with pytest.raises(ValueError, match="--name=value"):
        F.kaldi_fbank_options(tmp_path / "missing.conf")


# ------------------------------------------------------------------------------------------------------------ host bases
@pytest.mark.parametrize("sr,n_mels,low,high", [(16000, 80, 20.0, 0.0), (16000, 23, 20.0, 0.0), (8000, 40, 20.0, 0.0),
                                                (16000, 40, 100.0, -400.0), (16000, 40, 0.0, 7000.0)])
def test_mel_filters_match_oracle(F, sr, n_mels, low, high):
    N, S, P = R.sizes(sr)
    want = R.mel_bank(sr, P, n_mels, low, high)
    got = F.kaldi_mel_filters(sr, P, n_mels, low, high)
    assert got.shape == want.shape == (n_mels, P // 2) and got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    padded = F.kaldi_mel_basis(sr, P, n_mels, low, high)
    assert padded.shape == ((n_mels + 15) // 16 * 16, (P // 2 + 15) // 16 * 16) and padded.dtype == np.float32
    assert np.array_equal(padded[:n_mels, :P // 2], want.astype(np.float32)) and not padded[n_mels:].any()


def test_mel_bank_known_facts():
    bank = R.mel_bank(16000, 512, 80)
    cols = np.flatnonzero(bank.any(axis=0))
    assert not bank[:, 0].any() and cols[0] == 1 and cols[-1] == 255
    per = (bank > 0).sum(axis=1)
    assert per.min() >= 1 and per.max() <= 16
    assert bank.min() >= 0.0 and bank.max() <= 1.0


@pytest.mark.parametrize("kind", ["hamming", "hanning", "povey", "rectangular", "blackman"])
@pytest.mark.parametrize("N,P", [(400, 512), (200, 256), (37, 64)])
def test_dft_basis_matches_oracle(F, kind, N, P):
    w = R.window(N, kind)
    np.testing.assert_allclose(F.kaldi_window(N, kind), w, rtol=0, atol=1e-15)
    B = F.kaldi_dft_basis(N, P, kind)
    G = (P // 2 + 15) // 16
    KP = (N + 15) // 16 * 16
    assert B.shape == (32 * G, KP) and B.dtype == np.float32
    B = B.reshape(G, 2, 16, KP)
    # the oracle's transform: rfft of the windowed, zero-padded unit impulses
    eye = np.fft.rfft(np.concatenate([np.diag(w), np.zeros((N, P - N))], axis=1), axis=1)[:, :P // 2]  # (n, bin)
    cos = B[:, 0].reshape(16 * G, KP)
    sin = B[:, 1].reshape(16 * G, KP)
    np.testing.assert_allclose(cos[:P // 2, :N], eye.real.T, rtol=0, atol=2e-7)
    np.testing.assert_allclose(sin[:P // 2, :N], eye.imag.T, rtol=0, atol=2e-7)
    assert not cos[P // 2:].any() and not sin[P // 2:].any() and not B[..., N:].any()
    if kind == "hamming":  # symmetric, not the periodic window of features.dft_basis
        assert abs(w[0] - 0.08) < 1e-12 and abs(w[-1] - 0.08) < 1e-12 and np.allclose(w, w[::-1])


# ------------------------------------------------------------------------------------------------------------ oracle sanity
def test_oracle_frame_counts(F):
    N, S, P = R.sizes(16000)
    assert [R.n_frames(n, N, S) for n in (N - 1, N, N + S - 1, N + S)] == [0, 1, 1, 2]
    assert [F.kaldi_num_frames(n, N, S) for n in (N - 1, N, N + S - 1, N + S)] == [0, 1, 1, 2]
    assert list(F.kaldi_num_frames(np.array([N - 1, N, 16000]), N, S)) == [0, 1, 98]


def test_oracle_constant_signal_gives_the_floor():
    for kind in ("hamming", "povey"):
        out = R.fbank(np.full(2000, 700.0), window=kind, n_mels=80)
        assert out.shape == (11, 80) and np.all(out == FLOOR)
        out32 = R.fbank_f32(np.full(2000, 700.0), window=kind, n_mels=80)
        assert np.all(out32 == np.float32(FLOOR))
    assert abs(FLOOR + 15.9424) < 1e-4


def test_oracle_sine_peaks_in_its_filter():
    sr, n_mels = 16000, 80
    N, S, P = R.sizes(sr)
    lo, hi = R.mel(20.0), R.mel(8000.0)
    for hz in (300.0, 1330.0, 5000.0):
        y = 8000.0 * np.sin(2 * np.pi * hz * np.arange(4000) / sr)
        out = R.fbank(y, window="hamming", n_mels=n_mels)
        b = (R.mel(hz) - lo) / ((hi - lo) / (n_mels + 1))  # the filters whose support holds hz are floor(b) - 1 and floor(b)
        assert set(out.argmax(axis=1)) <= {int(b) - 1, int(b)}


def test_oracle_f32_model_is_close_and_probe_has_floor_frames():
    y = R.probe()
    want = R.fbank(y, window="hamming", n_mels=80)
    model = R.fbank_f32(y, window="hamming", n_mels=80)
    floor = np.all(want == FLOOR, axis=1)
    assert want.shape == (198, 80) and 20 <= floor.sum() <= 150
    assert np.array_equal(np.all(model == np.float32(FLOOR), axis=1), floor)
    assert np.abs(model - want).max() < 1e-3


def test_oracle_noise_is_standard_normal_and_keyed():
    g = R.noise(1234, 99, 40, 400)
    assert g.shape == (40, 400) and abs(g.mean()) < 4 / np.sqrt(g.size) and abs(g.std() - 1) < 0.02
    assert np.array_equal(g[3], R.frame_noise(1234, 99, 3, 400))
    assert not np.array_equal(g[3], R.frame_noise(1235, 99, 3, 400)) and not np.array_equal(g[3], R.frame_noise(1234, 98, 3, 400))
    assert not np.array_equal(g[3][160:], g[4][:240])  # overlapping frames do not share noise
    # Philox4x32-10 known answer (Random123 kat_vectors: counter 0, key 0)
    assert R.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert R.philox4x32_10((M := 0xFFFFFFFF, M, M, M), (M, M)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)


# ------------------------------------------------------------------------------------------------------------ ark / scp
def _entry(key, m):
    return key.encode() + b" " + b"\0B" + b"FM " + b"\4" + struct.pack("<i", m.shape[0]) + b"\4" + struct.pack("<i", m.shape[1]) + \
        m.astype("<f4").tobytes()


def test_ark_scp_bytes_and_round_trip(tmp_path):
    import kaldi_io_lite as K

    rng = np.random.default_rng(0)
    items = [("utt_a", rng.standard_normal((7, 80)).astype(np.float32)), ("spk1-utt_b", rng.standard_normal((1, 3)).astype(np.float32)),
             ("c", np.zeros((0, 80), np.float32)), ("d", rng.standard_normal((33, 80)).astype(np.float32))]
    ark, scp = tmp_path / "feats.ark", tmp_path / "feats.scp"
    assert K.write_ark_scp(str(ark), str(scp), items) == 4
    want = b"".join(_entry(k, m) for k, m in items)
    assert ark.read_bytes() == want
    lines = scp.read_text().splitlines()
    off = 0
    for (k, m), line in zip(items, lines):
        assert line == "%s %s:%d" % (k, ark, off + len(k) + 1)
        assert want[off + len(k) + 1:off + len(k) + 3] == b"\0B"
        got = K.load_mat(line.split(None, 1)[1])
        assert got.dtype == np.float32 and got.shape == m.shape and np.array_equal(got.view(np.uint32), m.view(np.uint32))
        off += len(_entry(k, m))
    back = list(K.read_ark(ark))
    assert [k for k, _ in back] == [k for k, _ in items] and all(np.array_equal(a, m) for (_, a), (_, m) in zip(back, items))
    K.write_len_scp(tmp_path / "len.scp", [(k, len(m)) for k, m in items])
    assert (tmp_path / "len.scp").read_text() == "utt_a 7\nspk1-utt_b 1\nc 0\nd 33\n"
    with pytest.raises(ValueError, match="key"):
        K.write_ark_scp(str(tmp_path / "x.ark"), str(tmp_path / "x.scp"), [("two words", items[0][1])])


def test_ark_double_compressed_and_text(tmp_path):
    import kaldi_io_lite as K

    m = np.arange(12, dtype=np.float64).reshape(3, 4) / 7
    p = tmp_path / "dm.ark"
    p.write_bytes(b"k1 \0BDM \4" + struct.pack("<i", 3) + b"\4" + struct.pack("<i", 4) + m.astype("<f8").tobytes())
    got = K.load_mat("%s:3" % p)
    assert got.dtype == np.float64 and np.array_equal(got, m)
    assert [(k, a.shape) for k, a in K.read_ark(p)] == [("k1", (3, 4))]
    for tok in (b"CM", b"CM2", b"CM3"):
        q = tmp_path / "cm.ark"
        q.write_bytes(b"k1 \0B" + tok + b" " + bytes(40))
        with pytest.raises(ValueError, match="compressed matrix \\(%s\\)" % tok.decode()) as e:
            K.load_mat("%s:3" % q)
        assert "cm.ark:3" in str(e.value)
    t = tmp_path / "text.ark"
    t.write_text("k1  [\n  1 2 3\n  4 5 6 ]\n")
    with pytest.raises(ValueError, match="text"):
        K.load_mat("%s:3" % t)
    with pytest.raises(ValueError, match="text"):
        list(K.read_ark(t))
    with pytest.raises(ValueError, match="piped"):
        K.load_mat("copy-feats ark:x.ark ark:- |")
    bare = tmp_path / "bare.mat"  # a matrix file without a key, read by path alone
    bare.write_bytes(_entry("k", m.astype(np.float32))[2:])
    assert np.array_equal(K.load_mat(str(bare)), m.astype(np.float32))


# ------------------------------------------------------------------------------------------------------------ the dataset
def test_kaldi_dataset_equals_numpy_dataset(tmp_path):
    import datasets as D
    import kaldi_io_lite as K

    rng = np.random.default_rng(5)
    mats = [("spk%d_u%d" % (j % 3, j), (rng.standard_normal((int(n), 12)) * 3 + 1).astype(np.float32))
            for j, n in enumerate((45, 20, 19, 88, 31))]
    K.write_ark_scp(str(tmp_path / "feats.ark"), str(tmp_path / "feats.scp"), mats)
    K.write_len_scp(tmp_path / "len.scp", [(k, len(m)) for k, m in mats])
    with open(tmp_path / "np.scp", "w") as fh:
        for k, m in mats:
            np.save(tmp_path / (k + ".npy"), m)
            fh.write("%s %s\n" % (k, tmp_path / (k + ".npy")))
    kd = D.KaldiDataset(tmp_path / "feats.scp", tmp_path / "len.scp", min_len=20, mvn_path=str(tmp_path / "mvn_k.json"), seg_len=20,
                        seg_shift=8)
    nd = D.NumpyDataset(tmp_path / "np.scp", tmp_path / "len.scp", min_len=20, mvn_path=str(tmp_path / "mvn_n.json"), seg_len=20,
                        seg_shift=8)
    assert isinstance(kd, D.NumpyDataset) and len(kd) == len(nd) == 4 and kd.num_segments == nd.num_segments > 10
    assert kd.seq_keys == nd.seq_keys and kd.seq_nsegs == nd.seq_nsegs
    for k in ("mean", "std"):
        assert np.array_equal(kd.mvn_params[k], nd.mvn_params[k])
    assert (tmp_path / "mvn_k.json").read_text() == (tmp_path / "mvn_n.json").read_text()
    for i in range(kd.num_segments):
        a, b = kd[i], nd[i]
        assert a[0] == b[0] and a[2] == b[2] and a[1].shape == (20, 12) and np.array_equal(a[1], b[1])
    for i in range(len(kd)):
        assert np.array_equal(kd.load_seq(i), nd.load_seq(i)) and kd.load_seq(i).dtype == np.float32


def test_cli_flags_and_wav_scp_rules(tmp_path):
    import eval_model
    import prepare_kaldi_data as PK
    import train_model

    assert train_model.build_parser().parse_args([]).data_format == "numpy"
    assert train_model.build_parser().parse_args(["--data-format", "kaldi"]).data_format == "kaldi"
    assert eval_model.build_parser().parse_args(["--checkpoint", "c", "--out", "o", "--data-format", "kaldi"]).data_format == "kaldi"
    a = PK.build_parser().parse_args(["data"])
    assert a.fbank_conf == "./misc/fbank.conf" and a.set_name is None and a.seed == 0 and not a.resample
    (tmp_path / "train").mkdir()
    (tmp_path / "train" / "wav.scp").write_text("u1 sph2pipe -f wav x.sph |\n")
    with pytest.raises(ValueError, match="piped"):
        PK.prepare_kaldi(tmp_path, "train", CONF)
    assert PK.main([str(tmp_path), "--set_name", "train", "--fbank_conf", str(tmp_path / "none.conf")]) == 1
    assert PK.READ_THREADS == 8


def test_read_wav_channel(F, tmp_path):
    from test_feats_cpu import _write_wav

    data = np.stack([np.arange(-50, 50), np.arange(100, 0, -1)], axis=1) * 100
    _write_wav(tmp_path / "st.wav", data, 16000, 2)
    y0, _ = F.read_wav(tmp_path / "st.wav", channel=0)
    y1, _ = F.read_wav(tmp_path / "st.wav", channel=1)
    ym, _ = F.read_wav(tmp_path / "st.wav")
    assert np.array_equal(y0 * 32768, data[:, 0]) and np.array_equal(y1 * 32768, data[:, 1])
    assert np.array_equal(ym, (y0 + y1) / np.float32(2))
    with pytest.raises(ValueError, match="channel 2"):
        F.read_wav(tmp_path / "st.wav", channel=2)


def test_short_utterance_is_a_host_error(F):
    with pytest.raises(ValueError, match="shorty.*399 samples"):
        F.compute_kaldi_fbank([np.zeros(16000, np.float32), np.zeros(399, np.float32)], CONF, names=["long", "shorty"])
    import zlib

    assert F.kaldi_stream_id("utt_a") == zlib.crc32(b"utt_a")
    with pytest.raises(ValueError, match="frame-length"):  # 2048-point frames do not fit the tile
        F.compute_kaldi_fbank([np.zeros(16000, np.float32)], {"frame-length": 100.0})


# ------------------------------------------------------------------------------------------------------------ the library
def test_symbols_and_argument_errors_before_launch(lib):
    import hip_binding as hb

    text = open(os.path.join(ROOT, "include", "fhvae_hip.h")).read()
    for name in ("fhvae_kaldi_fbank_fwd", "fhvae_kaldi_fbank_tile_rows"):
        assert name + "(" in text and hasattr(lib, name) and name in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    base = dict(wave=p, n_samples=4000, wave_ptr=p, frame_ptr=p, ids=p, U=1, n_frames=23, dft=p, mel=p, N=400, S=160, P=512, n_mels=80,
                preemph=0.97, dither=0.0, seed=0, flags=7, out=p, status=p)

    def call(**kw):
        a = dict(base, **kw)
        return lib.fhvae_kaldi_fbank_fwd(a["wave"], a["n_samples"], a["wave_ptr"], a["frame_ptr"], a["ids"], a["U"], a["n_frames"],
                                         a["dft"], a["mel"], a["N"], a["S"], a["P"], a["n_mels"], a["preemph"], a["dither"], a["seed"],
                                         a["flags"], a["out"], a["status"], None)

    for k in ("wave", "wave_ptr", "frame_ptr", "dft", "mel", "out", "status"):
        assert call(**{k: None}) == -1, k
    assert call(ids=None, dither=1.0) == -1          # dither needs the stream ids
    assert call(U=0) == -2 and call(n_frames=0) == -2 and call(n_samples=0) == -2
    assert call(S=0) == -2 and call(S=401) == -2     # 1 <= S <= N
    assert call(P=1024) == -2 and call(P=500) == -2  # P is the smallest power of two >= N
    assert call(N=1, P=1) == -2 and call(flags=8) == -2
    assert call(N=2049, P=4096, S=100) == -5         # P <= 2048
    assert call(n_mels=0) == -5 and call(n_mels=257) == -5
    unaligned = ctypes.c_void_p(p.value + 4)
    assert call(dft=unaligned) == -4 and call(mel=unaligned) == -4
    assert lib.fhvae_kaldi_fbank_tile_rows(400, 512, 80) in (16, 32, 48, 64)
    assert lib.fhvae_kaldi_fbank_tile_rows(200, 256, 40) == 64
    # P = 2048: the frame tile and the spectrum tile share the LDS up to N = FHVAE_KALDI_MAX_N
    assert lib.fhvae_kaldi_fbank_tile_rows(1504, 2048, 80) == 16 and lib.fhvae_kaldi_fbank_tile_rows(1505, 2048, 80) == 0
    assert call(N=1600, P=2048) == -5
    assert lib.fhvae_kaldi_fbank_tile_rows(400, 1024, 80) == 0 and lib.fhvae_kaldi_fbank_tile_rows(2049, 4096, 80) == 0
    assert lib.fhvae_kaldi_fbank_tile_rows(400, 512, 257) == 0 and lib.fhvae_kaldi_fbank_tile_rows(1, 1, 80) == 0
