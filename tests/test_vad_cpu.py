"""Energy VAD without a GPU: the oracle's own identities, the four entry points' argument errors (they return before any
launch), VAD_SIGNATURES against the declarations of include/fhvae_vad.h, the float-vector archive round trip, the errors of
kaldi_vad_options and of both prepare CLIs' new arguments."""
import ctypes
import os
import re

import numpy as np
import pytest

import vad_ref as R
import ext_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import vad

    return vad.load_library()


# ------------------------------------------------------------------------------------------------------------ the oracle
def test_oracle_without_context_is_the_plain_comparison():
    rng = np.random.default_rng(0)
    e = rng.uniform(0.0, 1.0, 300).astype(np.float32)
    for thr, scale, prop in ((0.0, 1.04 / 2, 1.0), (0.1, 0.5, 0.6), (-0.2, 1.3, 0.01)):
        vad, margin = R.decide(e, thr, scale, 0, prop, relative=False)
        th = thr + scale * (e.astype(np.float64).sum() / len(e))
        assert np.array_equal(vad, e.astype(np.float64) > th)
        assert np.array_equal(margin, np.abs(e.astype(np.float64) - th))


def test_oracle_all_equal_utterance_has_no_voiced_frame():
    # e > mean is false for every frame when all are equal: the sum of T equal float32 values is exact in float64
    for value in (0.0, 0.37, -15.942385):
        for T in (1, 7, 1000):
            for ctx in (0, 2):
                vad, _ = R.decide(np.full(T, value, dtype=np.float32), 0.0, 1.0, ctx, 0.12, relative=False)
                assert not vad.any()


def test_oracle_context_is_cut_at_the_utterance_edges():
    e = np.array([9, 0, 0, 0, 0, 0, 9], dtype=np.float32)  # mean 18 / 7: the two ends are above it
    vad, _ = R.decide(e, 0.0, 1.0, 2, 0.3, relative=False)
    # windows: t=0 -> [0, 2] 1 of 3; t=1 -> [0, 3] 1 of 4 (0.25 < 0.3); t=2 -> [0, 4] 1 of 5
    assert vad.tolist() == [True, False, False, False, False, False, True]
    vad, _ = R.decide(e, 0.0, 1.0, 2, 0.2, relative=False)
    assert vad.tolist() == [True, True, True, False, True, True, True]


def test_oracle_energies_on_known_signals():
    y = np.full(1000, 0.5, dtype=np.float32)
    e = R.rms_energy64(y, 400, 160)
    assert len(e) == R.rms_frames(1000, 400, 160) == 7 and np.allclose(e, 0.5, rtol=0, atol=1e-15)
    ramp = np.arange(551, dtype=np.float32)  # odd frame length: 275 reflected samples on either side
    e = R.rms_energy64(ramp, 551, 220)
    first = np.concatenate([ramp[275:0:-1], ramp[:276]]).astype(np.float64)
    assert len(e) == 3 and e[0] == np.sqrt(np.mean(first ** 2))
    le = R.log_energy64(np.full(560, 3.0), 400, 160, remove_dc=False)
    assert len(le) == 2 and np.allclose(le, np.log(3600.0), rtol=0, atol=1e-12)
    assert np.all(R.log_energy64(np.full(560, 3.0), 400, 160, remove_dc=True) == np.log(R.FLT_EPSILON))
    assert R.snip_frames(399, 400, 160) == 0 and R.snip_frames(559, 400, 160) == 1 and R.snip_frames(560, 400, 160) == 2


def test_the_test_signal_decides_far_from_its_thresholds():
    """The margins the GPU tests rely on: relative 1e-6 (RMS) and absolute 1e-5 (log energy, whose values are about 15 to 25) are
    about ten float32 roundings of a stored energy; the signal leaves a hundred times more."""
    for sr, n in ((16000, 19200), (8000, 9001), (22050, 30011)):
        vad, margin, _ = R.reference_vad(R.signal(sr, n), sr)
        assert margin.min() >= 1e-3 and 0 < vad.sum() < len(vad)
    vad, margin, _ = R.kaldi_vad(R.signal(16000, 19200))
    assert margin.min() >= 1e-3 and 0 < vad.sum() <= len(vad)


# ------------------------------------------------------------------------------------------------------------ the ABI
def test_signatures_match_the_header():
    import hip_binding as hb
    import vad as V

    text = ext_abi.header_text("fhvae_vad.h")
    found = ext_abi.declared("fhvae_vad.h", "fhvae_vad_")
    assert found == V.VAD_SIGNATURES
    assert sorted(found) == ["fhvae_vad_decide", "fhvae_vad_energy", "fhvae_vad_select", "fhvae_vad_ws_bytes"]
    assert not set(found) & set(hb.SIGNATURES)
    for name, value in (("MAX_FRAME", V.VAD_MAX_FRAME), ("MAX_CTX", V.VAD_MAX_CTX), ("CHUNK", V.VAD_CHUNK), ("TILE", V.VAD_TILE)):
        assert int(re.search(r"#define FHVAE_VAD_%s (\d+)" % name, text).group(1)) == value
    for name, value in (("RMS_CENTER", V.VAD_RMS_CENTER), ("LOGE_SNIP", V.VAD_LOGE_SNIP), ("REMOVE_DC", V.VAD_REMOVE_DC),
                        ("BAD_PTR", V.VAD_BAD_PTR), ("BAD_RANK", V.VAD_BAD_RANK)):
        assert int(re.search(r"FHVAE_VAD_%s = (\d+)" % name, text).group(1)) == value


def test_symbols_exported_and_errors_before_any_launch(lib):
    import hip_binding as hb
    import vad as V

    for name in V.VAD_SIGNATURES:
        assert hasattr(lib, name) and name not in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12 and len(hb.SIGNATURES) == 81
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    NULL, SHAPE, ALIGN, LIMIT = -1, -2, -4, -5

    swap = ext_abi.swap

    en = lib.fhvae_vad_energy
    #       wave n  wptr fptr U  nfr L    hop  mode flags energy status stream
    good = [p, 1000, p, p, 1, 7, 400, 160, 0, 0, p, p, None]
    for i in (0, 2, 3, 10, 11):  # wave, wave_ptr, frame_ptr, energy, status
        assert en(*swap(good, i, None)) == NULL
    for i, bad in ((1, 0), (1, -5), (4, 0), (4, -1), (5, -1), (6, 1), (6, 0), (7, 0), (7, -160), (8, 2), (8, -1), (9, 2), (9, 1)):
        assert en(*swap(good, i, bad)) == SHAPE, (i, bad)  # (flags = 1, REMOVE_DC, belongs to the log-energy mode only)
    assert en(*swap(good, 6, V.VAD_MAX_FRAME + 1)) == LIMIT and en(*swap(good, 7, 1 << 31)) == LIMIT
    assert en(*swap(good, 5, 0)) == 0  # n_frames == 0: nothing to do, nothing launched

    assert lib.fhvae_vad_ws_bytes(-1, 1) == SHAPE and lib.fhvae_vad_ws_bytes(1, -1) == SHAPE
    assert lib.fhvae_vad_ws_bytes(0, 0) == 8
    for n, U in ((1, 1), (1024, 1), (1025, 3), (360000, 1), (360000, 360)):
        assert lib.fhvae_vad_ws_bytes(n, U) == 8 * ((n // V.VAD_CHUNK + U) + U + -(-n // V.VAD_TILE) + 1)

    de = lib.fhvae_vad_decide
    need = lib.fhvae_vad_ws_bytes(7, 1)
    #       energy fptr U nfr thr  scale ctx prop ws ws_bytes vad rank status stream
    good = [p, p, 1, 7, 5.0, 0.5, 0, 0.6, p, need, p, p, p, None]
    for i in (0, 1, 8, 10, 11, 12):  # energy, frame_ptr, ws, vad, rank, status
        assert de(*swap(good, i, None)) == NULL
    for i, bad in ((2, 0), (2, -1), (3, -1), (6, -1), (7, 0.0), (7, -0.5), (7, 1.5), (7, float("nan")), (4, float("nan")),
                   (4, float("inf")), (5, float("-inf")), (9, need - 1), (9, 0)):
        assert de(*swap(good, i, bad)) == SHAPE, (i, bad)
    assert de(*swap(good, 6, V.VAD_MAX_CTX + 1)) == LIMIT
    assert de(*swap(good, 8, ctypes.c_void_p(p.value + 4))) == ALIGN
    assert de(*swap(good, 3, 0)) == 0

    se = lib.fhvae_vad_select
    #       rows vad rank nfr F  n_out out status stream
    good = [p, p, p, 7, 8, 3, p, p, None]
    for i in (0, 1, 2, 6, 7):  # rows, vad, rank, out, status
        assert se(*swap(good, i, None)) == NULL
    for i, bad in ((3, -1), (4, 0), (4, -8), (5, -1), (5, 8)):  # (n_out above n_frames)
        assert se(*swap(good, i, bad)) == SHAPE, (i, bad)
    assert se(*swap(good, 4, 1 << 31)) == LIMIT
    assert se(*swap(good, 5, 0)) == 0


# ------------------------------------------------------------------------------------------------------------ host side
def test_float_vector_archive_round_trip(tmp_path):
    import kaldi_io_lite as K

    vecs = [("utt-a", np.array([1, 0, 0, 1, 1], dtype=np.float32)), ("utt-b", np.zeros(0, dtype=np.float32)),
            ("ütt", np.arange(300, dtype=np.float32) % 2)]
    ark, scp = str(tmp_path / "vad.ark"), str(tmp_path / "vad.scp")
    assert K.write_vec_ark_scp(ark, scp, vecs) == 3
    got = list(K.read_vec_ark(ark))
    assert [k for k, _ in got] == [k for k, _ in vecs]
    for (_, a), (_, b) in zip(got, vecs):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    lines = [ln.split(None, 1) for ln in open(scp).read().splitlines()]
    assert [k for k, _ in lines] == [k for k, _ in vecs]
    for (_, spec), (_, b) in zip(lines, vecs):
        assert np.array_equal(K.load_vec(spec), b)
    raw = open(ark, "rb").read()
    assert raw.startswith(b"utt-a \0BFV \4\5\0\0\0")  # what compute-vad-decision writes
    with pytest.raises(ValueError, match="1-D"):
        K.write_vec_ark_scp(ark, scp, [("k", np.zeros((2, 2)))])
    with pytest.raises(ValueError, match="not a Kaldi key"):
        K.write_vec_ark_scp(ark, scp, [("a b", np.zeros(2))])
    K.write_ark_scp(ark, scp, [("m", np.zeros((2, 3), dtype=np.float32))])
    with pytest.raises(ValueError, match="not a vector token"):
        list(K.read_vec_ark(ark))
    open(ark, "wb").write(b"k \0BFV \4\5\0\0\0\0\0")
    with pytest.raises(ValueError, match="ends inside a vector"):
        list(K.read_vec_ark(ark))
    open(ark, "wb").write(b"k 1 0 1")
    with pytest.raises(ValueError, match="not a binary Kaldi vector"):
        list(K.read_vec_ark(ark))


def test_kaldi_vad_options(tmp_path):
    import features as F

    assert F.kaldi_vad_options() == {"vad-energy-threshold": 5.0, "vad-energy-mean-scale": 0.5, "vad-frames-context": 0,
                                     "vad-proportion-threshold": 0.6}
    conf = tmp_path / "vad.conf"
    conf.write_text("# the recipes' settings\n--vad-energy-threshold=5.5\n--vad-energy-mean-scale=0.5  # half the mean\n\n"
                    "--vad-frames-context=2\n--vad-proportion-threshold=0.12\n")
    assert F.kaldi_vad_options(str(conf)) == {"vad-energy-threshold": 5.5, "vad-energy-mean-scale": 0.5, "vad-frames-context": 2,
                                              "vad-proportion-threshold": 0.12}
    assert F.kaldi_vad_options({"vad_frames_context": 3})["vad-frames-context"] == 3
    with pytest.raises(ValueError, match="cannot read the Kaldi VAD configuration"):
        F.kaldi_vad_options(str(tmp_path / "missing.conf"))
    for text, match in (("--vad-energy-treshold=5\n", "unknown option --vad-energy-treshold"),
                        ("--num-mel-bins=80\n", "unknown option --num-mel-bins"),
                        ("vad-frames-context=2\n", "is not an option"),
                        ("--vad-frames-context=2.5\n", "not a int"),
                        ("--vad-energy-threshold=high\n", "not a float"),
                        ("--vad-energy-threshold\n", "not a float"),
                        ("--vad-frames-context=-1\n", "frames context"),
                        ("--vad-frames-context=5000\n", "frames context"),
                        ("--vad-proportion-threshold=0\n", "proportion threshold"),
                        ("--vad-proportion-threshold=1.5\n", "proportion threshold"),
                        ("--vad-energy-mean-scale=nan\n", "must be finite")):
        conf.write_text(text)
        with pytest.raises(ValueError, match=match) as err:
            F.kaldi_vad_options(str(conf))
        assert str(conf) in str(err.value)
    with pytest.raises(ValueError, match="unknown option"):
        F.kaldi_vad_options({"dither": 0})
    with pytest.raises(ValueError, match="vad must be a dict"):
        F.compute_features([], 16000, vad="drop")
    with pytest.raises(ValueError, match="vad must be a dict"):
        F.compute_kaldi_fbank([], vad={"th_ratio": 0.5})
    assert F.compute_features([], 16000, vad={"drop": True}) == ([], [])
    assert F.compute_kaldi_fbank([], vad={}) == ([], [])
    with pytest.raises(ValueError, match="proportion threshold"):
        F.vad_decide([np.zeros(3)], 5.0, 0.5, 0, 0.0)
    assert F.vad_decide([], 5.0, 0.5, 0, 0.6) == []


def test_cli_argument_errors(tmp_path, capsys):
    import prepare_kaldi_data as PK
    import prepare_numpy_data as PN

    for mod, argv in ((PN, [str(tmp_path), "--vad", "keep"]), (PN, [str(tmp_path), "--vad_th_ratio", "0.5"]),
                      (PN, [str(tmp_path), "--vad", "mark", "--vad_th_ratio", "nan"]), (PK, [str(tmp_path), "--vad", "keep"]),
                      (PK, [str(tmp_path), "--vad_conf", "vad.conf"])):
        with pytest.raises(SystemExit) as e:
            mod.main(argv)
        assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--vad_th_ratio needs --vad" in err and "--vad_conf needs --vad" in err and "--vad_th_ratio must be finite" in err
    assert PN.build_parser().parse_args(["d"]).vad is None and PK.build_parser().parse_args(["d"]).vad is None
    # a bad VAD configuration is reported before any file is read
    (tmp_path / "train").mkdir()
    (tmp_path / "train" / "wav.scp").write_text("")
    fbank = tmp_path / "fbank.conf"
    fbank.write_text("--num-mel-bins=80\n")
    bad = tmp_path / "vad.conf"
    bad.write_text("--vad-frames-context=two\n")
    assert PK.main([str(tmp_path), "--set_name", "train", "--fbank_conf", str(fbank), "--vad", "drop", "--vad_conf", str(bad)]) == 1
    assert "--vad-frames-context" in capsys.readouterr().err
    with pytest.raises(ValueError, match="vad must be one of"):
        PN.prepare_numpy("librispeech", "train", str(tmp_path), vad="keep")
    with pytest.raises(ValueError, match="vad must be one of"):
        PK.prepare_kaldi(str(tmp_path), "train", str(fbank), vad="keep")
