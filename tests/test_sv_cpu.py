"""Speaker verification without a GPU: the EER read off histograms, the speaker tables, the host-side refusals of
fhvae_sv_hist and eval_model.py's option rules."""
import ctypes

import numpy as np
import pytest

import sv_ref as R


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding as hb

    return hb.load_library()


def test_eer_separated_classes_is_zero():
    import verification as V

    h = np.zeros((2, 64), dtype=np.int64)
    h[1, 3:20] = 5   # non-targets low
    h[0, 40:60] = 2  # targets high
    r = V.eer_from_hist(h)
    assert r["eer"] == 0.0 and r["n_target"] == 40 and r["n_nontarget"] == 85
    # the first edge at which no non-target is accepted any more
    assert r["threshold"] == -1.0 + 2.0 * 20 / 64


def test_eer_identical_classes_is_half():
    import verification as V

    rs = np.random.RandomState(0)
    row = rs.randint(0, 50, size=128)
    r = V.eer_from_hist(np.stack([row, row]).astype(np.uint64))
    assert abs(r["eer"] - 0.5) <= 1e-12


def test_eer_hand_worked_interpolation():
    import verification as V

    # bins:          0    1    2    3          n
    # targets        1    1    4    4         10
    # non-targets    4    3    2    1         10
    # edge k         0    1    2    3    4
    # FRR(k)         0   .1   .2   .6    1     targets in bins < k
    # FAR(k)         1   .6   .3   .1    0     non-targets in bins >= k
    # FRR - FAR     -1  -.5  -.1  +.5   +1     first k with FRR >= FAR: 3
    # t = .1 / (.5 + .1) = 1/6;  EER = .2 + (.6 - .2) / 6 = .3 + (.1 - .3) / 6 = 4/15
    # threshold: edge 2 + 1/6 of a bin = -1 + 2 (2 + 1/6) / 4 = 1/12;  bin 2 holds 4/10 of the targets + 2/10 of the non-targets
    r = V.eer_from_hist([[1, 1, 4, 4], [4, 3, 2, 1]])
    assert abs(r["eer"] - 4.0 / 15.0) <= 1e-12
    assert abs(r["threshold"] - 1.0 / 12.0) <= 1e-12
    assert abs(r["crossing_mass"] - 0.6) <= 1e-12
    assert r["n_target"] == 10 and r["n_nontarget"] == 10


def test_eer_counts_beyond_int64_do_not_wrap():
    import verification as V

    h = np.array([[0, 0, 2 ** 63, 2 ** 63], [2 ** 63, 2 ** 63, 0, 0]], dtype=np.uint64)
    r = V.eer_from_hist(h)
    assert r["eer"] == 0.0 and r["n_target"] == 2 ** 64


def test_eer_empty_classes_raise():
    import verification as V

    with pytest.raises(ValueError, match="no target trials"):
        V.eer_from_hist([[0, 0, 0, 0], [1, 2, 3, 4]])
    with pytest.raises(ValueError, match="no non-target trials"):
        V.eer_from_hist([[1, 2, 3, 4], [0, 0, 0, 0]])
    with pytest.raises(ValueError, match="no target trials"):
        V.eer_from_hist(np.zeros((2, 64), dtype=np.int64))
    with pytest.raises(ValueError, match=r"\(2, NB\)"):
        V.eer_from_hist(np.zeros((3, 64), dtype=np.int64))


def test_oracle_eer_agrees_with_histogram_of_its_own_scores():
    """The oracle against eer_from_hist, no kernel involved: the histogram EER lies within crossing_mass of the exact one."""
    import verification as V

    emb, label = R.make_case(120, 16, 6, 7)
    tar, non = R.trial_scores(emb, label)
    for NB in (64, 1024):
        r = V.eer_from_hist(R.hist_ref(emb, label, NB))
        assert r["n_target"] == len(tar) and r["n_nontarget"] == len(non)
        assert abs(r["eer"] - R.exact_eer(tar, non)) <= r["crossing_mass"]


def test_read_utt2spk(tmp_path):
    import verification as V

    f = tmp_path / "utt2spk"
    f.write_text("103-1240-0000 103\n103-1240-0001 103\n\nFADG0_SA1   FADG0\n")
    assert V.read_utt2spk(f) == {"103-1240-0000": "103", "103-1240-0001": "103", "FADG0_SA1": "FADG0"}
    f.write_text("a spk1\nb\n")
    with pytest.raises(ValueError, match=r"utt2spk:2: expected `<seq> <spk>`"):
        V.read_utt2spk(f)
    f.write_text("a spk1\na spk2\n")
    with pytest.raises(ValueError, match="listed twice"):
        V.read_utt2spk(f)
    with pytest.raises(OSError):
        V.read_utt2spk(tmp_path / "missing")


def test_speakers_from_keys():
    import verification as V

    assert V.speakers_from_keys(["103-1240-0000", "103-1241-0003", "1034-121119-0049"], "-") == ["103", "103", "1034"]
    assert V.speakers_from_keys(["FADG0_SA1", "MABW0_SX134", "FADG0_SI649"], "_") == ["FADG0", "MABW0", "FADG0"]
    with pytest.raises(ValueError, match="'FADG0_SA1'"):
        V.speakers_from_keys(["103-1240-0000", "FADG0_SA1"], "-")
    with pytest.raises(ValueError, match="'-abc'"):
        V.speakers_from_keys(["-abc"], "-")
    with pytest.raises(ValueError, match="separator is empty"):
        V.speakers_from_keys(["abc"], "")
    labels, n = V.labels_from_speakers(["b", None, "a", "b"])
    assert labels.dtype == np.int32 and labels.tolist() == [1, -1, 0, 1] and n == 2


def test_host_side_refusals(lib):
    """Argument errors come back as negative codes before anything touches a GPU."""
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(emb=p, ld=32, label=p, S=8, D=32, nb=1024, ws=p, wsb=4096, hist=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.fhvae_sv_hist(a["emb"], a["ld"], a["label"], a["S"], a["D"], a["nb"], a["ws"], a["wsb"], a["hist"], None)

    for name in ("emb", "label", "ws", "hist"):
        assert call(**{name: None}) == -1, name
    assert call(D=24, ld=24) == -2       # not a multiple of 16
    assert call(D=144, ld=144) == -2     # beyond the widest instantiation
    assert call(D=0) == -2
    assert call(nb=100) == -2            # not a power of two
    assert call(nb=16384) == -2
    assert call(nb=32) == -2
    assert call(S=0) == -2
    assert call(ld=16) == -2             # ld < D
    assert call(ld=34) == -4             # rows not 16-byte aligned
    assert call(emb=ctypes.c_void_p(p.value + 4)) == -4
    assert call(wsb=16) == -2            # workspace too small
    assert call(S=(1 << 24) + 1, wsb=1 << 40) == -5
    assert lib.fhvae_sv_hist_ws_bytes(0) == 0 and lib.fhvae_sv_hist_ws_bytes(1) == 256
    assert lib.fhvae_sv_hist_ws_bytes(100000) >= 400000


def test_eval_model_speaker_option_rules(capsys):
    import eval_model as EM

    base = ["--checkpoint", "c", "--out", "o"]
    with pytest.raises(SystemExit) as e:
        EM.parse_args(base + ["--feat-scp", "f", "--utt2spk", "u", "--spk-key-sep", "-"])
    assert e.value.code == 2 and "not allowed with" in capsys.readouterr().err
    for opt in (["--utt2spk", "u"], ["--spk-key-sep", "-"]):
        with pytest.raises(SystemExit) as e:
            EM.parse_args(base + opt)
        assert e.value.code == 2 and "--feat-scp" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        EM.parse_args(base + ["--feat-scp", "f", "--spk-key-sep", "-", "--sv-bins", "1000"])
    capsys.readouterr()
    a = EM.parse_args(base + ["--feat-scp", "f", "--spk-key-sep", "-"])
    assert a.spk_key_sep == "-" and a.utt2spk is None and a.sv_bins == 4096
    a = EM.parse_args(base)
    assert a.spk_key_sep is None and a.utt2spk is None
