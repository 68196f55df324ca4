"""Cepstra, deltas and sliding CMVN without a GPU: KPOST_SIGNATURES against the declarations of include/fhvae_kaldi_post.h, the
entry points' argument errors (they return before any launch), the host-side constants (DCT matrix, delta scales), the window
rule against a brute-force transcription, the MFCC option parser, and the errors of the command lines' new arguments."""
import ctypes
import os
import re

import numpy as np
import pytest

import kaldi_post_ref as R
import ext_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import kaldi_post

    return kaldi_post.load_library()


# ------------------------------------------------------------------------------------------------------------ the ABI
def test_signatures_match_the_header():
    import hip_binding as hb
    import kaldi_post as KP

    text = ext_abi.header_text("fhvae_kaldi_post.h")
    found = ext_abi.declared("fhvae_kaldi_post.h", "fhvae_kaldi_")
    assert found == KP.KPOST_SIGNATURES
    assert sorted(found) == ["fhvae_kaldi_add_deltas", "fhvae_kaldi_cepstra", "fhvae_kaldi_cmvn_sliding", "fhvae_kaldi_post_ws_bytes"]
    assert not set(found) & set(hb.SIGNATURES)
    for name, value in (("MAX_BINS", KP.KPOST_MAX_BINS), ("MAX_WINDOW", KP.KPOST_MAX_WINDOW), ("MAX_COLS", KP.KPOST_MAX_COLS),
                        ("CHUNK", KP.KPOST_CHUNK)):
        assert int(re.search(r"#define FHVAE_KPOST_%s (\d+)" % name, text).group(1)) == value
    assert int(re.search(r"FHVAE_KPOST_BAD_PTR = (\d+)", text).group(1)) == KP.KPOST_BAD_PTR
    assert R.CHUNK == KP.KPOST_CHUNK


def test_the_main_header_is_unchanged(lib):
    import hip_binding as hb
    import kaldi_post as KP

    text = open(os.path.join(ROOT, "include", "fhvae_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(fhvae_[a-z0-9_]+)\s*\(", text))
    assert names == set(hb.SIGNATURES) and len(names) == 81 and lib.fhvae_abi_version() == 12
    assert not names & set(KP.KPOST_SIGNATURES)


def test_symbols_exported_and_errors_before_any_launch(lib):
    import kaldi_post as KP

    for name in KP.KPOST_SIGNATURES:
        assert hasattr(lib, name)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    NULL, SHAPE, ALIGN, LIMIT = -1, -2, -4, -5
    inf = float("inf")

    swap = ext_abi.swap

    ce = lib.fhvae_kaldi_cepstra
    #       logmel ld  n  B   dct C  lifter energy floor out stream
    good = [p, 23, 7, 23, p, 13, p, p, -inf, p, None]
    for i in (0, 4, 9):  # logmel, dct, out (lifter and energy may be NULL)
        assert ce(*swap(good, i, None)) == NULL
    for i, bad in ((1, 22), (2, -1), (3, 0), (5, 0), (5, 24), (8, float("nan"))):  # ld < B, C > B
        assert ce(*swap(good, i, bad)) == SHAPE, (i, bad)
    assert ce(p, 129, 7, 129, p, 13, None, None, -inf, p, None) == LIMIT  # B > 128
    assert ce(*swap(good, 2, 0)) == 0  # n == 0: nothing to do, nothing launched

    de = lib.fhvae_kaldi_add_deltas
    #       in fptr U  n  D  order window scales out status stream
    good = [p, p, 1, 7, 13, 2, 2, p, p, p, None]
    for i in (0, 1, 7, 8, 9):  # in, frame_ptr, scales, out, status
        assert de(*swap(good, i, None)) == NULL
    for i, bad in ((2, 0), (2, -1), (3, -1), (4, 0), (5, 0), (5, 3), (6, 0), (6, -2)):  # order 3, window 0
        assert de(*swap(good, i, bad)) == SHAPE, (i, bad)
    assert de(*swap(good, 6, 9)) == LIMIT  # window 9
    assert de(*swap(good, 4, 342)) == LIMIT and de(*swap(swap(good, 4, 513), 5, 1)) == LIMIT  # (order + 1) D > 1024
    assert de(*swap(good, 3, 0)) == 0

    wb = lib.fhvae_kaldi_post_ws_bytes
    assert wb(-1, 1, 13) == SHAPE and wb(1, -1, 13) == SHAPE and wb(1, 1, 0) == SHAPE and wb(1, 1, 1025) == LIMIT
    for n, U, D in ((1, 1, 13), (256, 1, 39), (257, 3, 13), (360000, 1, 80), (360000, 360, 13)):
        assert wb(n, U, D) == 2 * (n // KP.KPOST_CHUNK + 2 * U) * D * 16

    cm = lib.fhvae_kaldi_cmvn_sliding
    need = wb(7, 1, 13)
    big = (ctypes.c_double * (need // 8 + 1))()
    w = ctypes.cast(big, ctypes.c_void_p)
    q = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
    #       in fptr U  n  D   cmn  min center norm ws ws_bytes out status stream
    good = [p, p, 1, 7, 13, 300, 100, 1, 0, w, need, q, p, None]
    for i in (0, 1, 9, 11, 12):  # in, frame_ptr, ws, out, status
        assert cm(*swap(good, i, None)) == NULL
    for i, bad in ((2, 0), (3, -1), (4, 0), (5, 0), (5, -300), (6, 0), (7, 2), (8, -1), (10, need - 1), (10, 0), (11, p)):
        assert cm(*swap(good, i, bad)) == SHAPE, (i, bad)  # cmn_window 0, a workspace too small, out aliasing in
    assert cm(*swap(good, 4, 1025)) == LIMIT and cm(*swap(good, 5, 1 << 31)) == LIMIT
    assert cm(*swap(good, 9, ctypes.c_void_p(w.value + 4))) == ALIGN
    assert cm(*swap(good, 3, 0)) == 0


# ------------------------------------------------------------------------------------------------------------ host side
@pytest.mark.parametrize("B", [23, 40, 80])
def test_dct_matrix_is_orthonormal(B):
    import kaldi_post as KP

    d = KP.dct_matrix(B, B)
    assert d.dtype == np.float32 and d.shape == (B, B)
    assert np.abs(d.astype(np.float64) @ d.astype(np.float64).T - np.eye(B)).max() <= 1e-6
    assert np.array_equal(d[:13], KP.dct_matrix(13, B))
    assert np.array_equal(d, R.dct64(B, B).astype(np.float32))
    assert np.array_equal(KP.lifter_coeffs(13, 22.0), R.lifter64(13, 22.0).astype(np.float32))
    assert KP.lifter_coeffs(13, 22.0)[0] == 1.0


def test_delta_scales():
    import kaldi_post as KP

    s = KP.delta_scales(2, 2)
    assert [len(v) for v in s] == [1, 5, 9] and all(v.dtype == np.float32 for v in s)
    assert np.array_equal(s[0], np.float32([1]))
    assert np.array_equal(s[1], np.float32([-.2, -.1, 0, .1, .2]))
    assert np.array_equal(s[2], np.float32([.04, .04, .01, -.04, -.1, -.04, .01, .04, .04]))
    for order, window in ((1, 1), (2, 3), (2, 8)):
        got, want = KP.delta_scales(order, window), R.scales64(order, window)
        assert [len(v) for v in got] == [2 * i * window + 1 for i in range(order + 1)]
        for a, b in zip(got, want):
            assert np.array_equal(a, b.astype(np.float32))
            assert abs(float(b.sum())) < 1e-12 or len(b) == 1  # a delta of a constant is 0


def _brute_window(t, T, W, M, center):
    """The rule of include/fhvae_kaldi_post.h, transcribed a second time (tuple assignments, no early exits)."""
    if center:
        lo, hi = t - W // 2, t - W // 2 + W
    else:
        lo, hi = t - W, t + 1
    if lo < 0:
        hi, lo = hi - lo, 0
    if not center and hi > t:
        hi = max(t + 1, M)
    if hi > T:
        lo, hi = max(lo - (hi - T), 0), T
    return lo, hi


@pytest.mark.parametrize("center", [True, False])
def test_cmvn_window(center):
    import kaldi_post as KP

    for T in (1, 2, 99, 100, 101, 299, 300, 301, 700):
        for W, M in ((300, 100), (600, 100), (20000, 100), (1, 1), (7, 50)):
            prev = (0, 0)
            for t in range(T):
                b, e = KP.cmvn_window(t, T, W, M, center)
                assert (b, e) == _brute_window(t, T, W, M, center) == R.window(t, T, W, M, center)
                assert 0 <= b < e <= T, (t, T, W, M, b, e)
                if center:
                    assert e - b == min(T, W)
                else:
                    assert b <= t < e  # a causal window holds its frame
                # what the kernel's tiles rely on: b and e rise by at most one per frame
                assert 0 <= b - prev[0] <= 1 or t == 0
                assert 0 <= e - prev[1] <= 1 or t == 0
                prev = (b, e)
    assert KP.cmvn_window(5, 700, 20000, 100, True) == (0, 700)  # per-utterance CMVN


def test_mfcc_options(tmp_path):
    import features as F
    import kaldi_post as KP

    o = KP.kaldi_mfcc_options()
    assert (o["num-mel-bins"], o["num-ceps"], o["cepstral-lifter"], o["use-energy"], o["energy-floor"], o["raw-energy"]) == (
        23, 13, 22.0, True, 0.0, True)
    frame = [k for k in F.KALDI_DEFAULTS if k not in KP.MFCC_DEFAULTS and k not in KP.MFCC_NOT_OPTIONS]
    assert {k: o[k] for k in frame} == {k: F.KALDI_DEFAULTS[k] for k in frame} and set(o) == set(frame) | set(KP.MFCC_DEFAULTS)
    assert KP.kaldi_mfcc_options(o) == o  # (its own result is a valid source)
    assert F.kaldi_fbank_options(KP.fbank_part(o))["use-energy"] is False  # the bank in front is a plain fbank
    conf = tmp_path / "mfcc.conf"
    conf.write_text("# a recipe's settings\n--use-energy=false  # C0 from the DCT\n--num-mel-bins=40\n--num-ceps=20\n--cepstral-lifter=0\n"
                    "--sample-frequency=8000\n--low-freq=40\n--dither=0\n")
    o = KP.kaldi_mfcc_options(str(conf))
    assert (o["use-energy"], o["num-mel-bins"], o["num-ceps"], o["cepstral-lifter"], o["sample-frequency"], o["low-freq"], o["dither"]) == (
        False, 40, 20, 0.0, 8000.0, 40.0, 0.0)
    assert KP.kaldi_mfcc_options({"num_ceps": 5, "energy-floor": 1.5})["num-ceps"] == 5
    with pytest.raises(ValueError, match="cannot read the Kaldi MFCC configuration"):
        KP.kaldi_mfcc_options(str(tmp_path / "missing.conf"))
    for text, match in (("--htk-compat=true\n", "--htk-compat=true is not supported"),
                        ("--raw-energy=false\n", "--raw-energy=false is not supported"),
                        ("--num-ceps=24\n", "--num-ceps=24 is outside"),
                        ("--num-ceps=0\n", "--num-ceps=0 is outside"),
                        ("--num-mel-bins=12\n", "--num-ceps=13 is outside"),
                        ("--num-mel-bins=200\n--num-ceps=13\n", "--num-mel-bins=200 is above 128"),
                        ("--num-ceps=12.5\n", "--num-ceps has the value '12.5', not a int"),
                        ("--cepstral-lifter=big\n", "--cepstral-lifter has the value 'big', not a float"),
                        ("--use-energy=maybe\n", "--use-energy has the value 'maybe', not a bool"),
                        ("--snip-edges=false\n", "--snip-edges=false is not supported"),
                        ("--round-to-power-of-two=false\n", "--round-to-power-of-two=false is not supported"),
                        ("--vtln-low=100\n", "--vtln-low is not supported"),
                        ("--use-log-fbank=true\n", "unknown option --use-log-fbank"),
                        ("--use-power=false\n", "unknown option --use-power"),
                        ("--num-cepstra=13\n", "unknown option --num-cepstra"),
                        ("--window-type=kaiser\n", "--window-type=kaiser"),
                        ("num-ceps=13\n", "is not an option")):
        conf.write_text(text)
        with pytest.raises(ValueError, match=match) as err:
            KP.kaldi_mfcc_options(str(conf))
        assert str(conf) in str(err.value), str(err.value)
    for order, window in ((0, 2), (3, 2), (2, 0), (2, 9)):
        with pytest.raises(ValueError, match="--delta-"):
            KP.deltas_spec(order, window)
    for cw, mw in ((0, 100), (300, 0), (1 << 31, 100)):
        with pytest.raises(ValueError, match="--cmn-"):
            KP.cmvn_spec(cw, mw)
    assert KP.compute_kaldi_mfcc([]) == [] and KP.post_process([], KP.deltas_spec()) == []
    with pytest.raises(ValueError, match="kind must be"):
        KP.compute_kaldi_feats([], kind="plp")


def test_oracle_identities():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((40, 3)).astype(np.float32)
    # deltas of a ramp: the first order is the slope away from the edges, the second is 0
    ramp = np.arange(40, dtype=np.float64)[:, None] * np.array([[1.0, -2.0, 0.5]])
    out, _ = R.add_deltas(ramp, R.scales64(2, 2))
    assert np.allclose(out[2:-2, 3:6], [[1.0, -2.0, 0.5]], atol=1e-12) and np.allclose(out[4:-4, 6:], 0.0, atol=1e-12)
    assert np.array_equal(out[:, :3], ramp)
    # per-utterance CMVN: zero mean, unit variance
    y = R.cmvn_sliding(x, 20000, 100, True, True).astype(np.float64)
    assert np.abs(y.mean(axis=0)).max() < 1e-6 and np.abs(y.var(axis=0) - 1.0).max() < 1e-5
    # the two-level prefix is the plain prefix up to rounding, and exact on integers
    ints = rng.integers(-1000, 1000, (700, 2)).astype(np.float64)
    assert np.array_equal(R._prefix(ints)[1:], np.cumsum(ints, axis=0))
    # a window of one frame without centring never occurs; with norm_vars and one frame the variance is 1
    assert np.array_equal(R.cmvn_sliding(x[:1], 300, 100, True, True), np.zeros((1, 3), dtype=np.float32))


# ------------------------------------------------------------------------------------------------------------ command lines
def test_cli_argument_errors(tmp_path, capsys):
    import postprocess_kaldi_feats as PP
    import prepare_kaldi_data as PK

    io = ["--feat-scp", str(tmp_path / "in" / "feats.scp"), "--len-scp", str(tmp_path / "in" / "len.scp"), "--out", str(tmp_path / "out")]
    for mod, argv, text in ((PK, [str(tmp_path), "--delta-order", "1"], "need --add-deltas"),
                            (PK, [str(tmp_path), "--delta-window", "3"], "need --add-deltas"),
                            (PK, [str(tmp_path), "--cmn-window", "600"], "need --cmvn-sliding"),
                            (PK, [str(tmp_path), "--no-cmn-center"], "need --cmvn-sliding"),
                            (PK, [str(tmp_path), "--cmn-norm-vars", "--add-deltas"], "need --cmvn-sliding"),
                            (PK, [str(tmp_path), "--add-deltas", "--delta-order", "3"], "--delta-order 3 is not 1 or 2"),
                            (PK, [str(tmp_path), "--add-deltas", "--delta-window", "9"], "--delta-window 9 is outside"),
                            (PK, [str(tmp_path), "--cmvn-sliding", "--cmn-window", "0"], "--cmn-window 0 is outside"),
                            (PK, [str(tmp_path), "--mfcc_conf", "m.conf", "--fbank_conf", "f.conf"], "exclude each other"),
                            (PP, io, "nothing to do"),
                            (PP, io + ["--delta-order", "1"], "need --add-deltas"),
                            (PP, io + ["--cmvn-sliding", "--cmn-min-window", "0"], "--cmn-min-window 0 is outside"),
                            (PP, io[:4] + ["--out", str(tmp_path / "in"), "--add-deltas"], "would be overwritten"),
                            (PP, io[2:] + ["--add-deltas"], "--feat-scp")):
        with pytest.raises(SystemExit) as e:
            mod.main(argv)
        assert e.value.code == 2
        assert text in capsys.readouterr().err, (argv, text)
    a = PK.build_parser().parse_args(["d"])
    assert a.mfcc_conf is None and not a.add_deltas and not a.cmvn_sliding
    # a bad MFCC configuration is reported before any file is read, and the fbank file is not opened
    (tmp_path / "train").mkdir()
    (tmp_path / "train" / "wav.scp").write_text("")
    bad = tmp_path / "mfcc.conf"
    bad.write_text("--htk-compat=true\n")
    assert PK.main([str(tmp_path), "--set_name", "train", "--mfcc_conf", str(bad)]) == 1
    assert "--htk-compat=true is not supported" in capsys.readouterr().err
    bad.write_text("--num-ceps=13\n")
    assert PK.main([str(tmp_path), "--set_name", "train", "--mfcc_conf", str(bad), "--add-deltas", "--cmvn-sliding"]) == 0  # (no utterance)
    # the argument list main() prints is the old one when no new flag is given
    out = capsys.readouterr().out
    assert "add_deltas=True" in out and "cmvn_sliding=True" in out and "delta_order" not in out
    fb = tmp_path / "fbank.conf"
    fb.write_text("--num-mel-bins=80\n")
    assert PK.main([str(tmp_path), "--set_name", "train", "--fbank_conf", str(fb)]) == 0
    out = capsys.readouterr().out
    assert "vad_conf=None)" in out and "mfcc_conf" not in out and "add_deltas" not in out
    # postprocess: a key without a length, a row count that differs
    import kaldi_io_lite as K

    (tmp_path / "in").mkdir()
    K.write_ark_scp(str(tmp_path / "in" / "feats.ark"), io[1], [("a", np.zeros((5, 4), dtype=np.float32)), ("b", np.ones((3, 4), dtype=np.float32))])
    K.write_len_scp(io[3], [("a", 5)])
    assert PP.main(io + ["--add-deltas"]) == 1
    assert "b has no entry" in capsys.readouterr().err
    K.write_len_scp(io[3], [("a", 4), ("b", 3)])
    with pytest.raises(ValueError, match="a: 5 rows"):  # (checked before anything is uploaded)
        PP.postprocess(io[1], io[3], io[5], {"order": 2, "window": 2})
