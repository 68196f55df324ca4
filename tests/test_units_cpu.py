"""Units without a GPU: KM_SIGNATURES against include/fhvae_kmeans.h, the entry points' export and their argument errors (they
return before any launch), the workspace size, the oracle (tests/kmeans_ref.py) on cases worked by hand, units.unit_quality /
bitrate / frame_phones / write_units, and the command lines' argument errors."""
import math
import os
import re

import numpy as np
import pytest

import kmeans_ref as R
import ext_abi
from ext_abi import aligned as _aligned, swap as _swap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, ALIGN, LIMIT = -1, -2, -4, -5


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import units

    return units.load_library()


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_signatures_match_the_header():
    import hip_binding as hb
    import units

    text = ext_abi.header_text("fhvae_kmeans.h")
    found = ext_abi.declared("fhvae_kmeans.h", "fhvae_km_")
    assert found == units.KM_SIGNATURES and sorted(found) == ["fhvae_km_assign", "fhvae_km_update", "fhvae_km_ws_bytes"]
    assert not set(found) & set(hb.SIGNATURES)
    for name, value in (("PIECE", units.KM_PIECE), ("MAX_ROWS", units.KM_MAX_ROWS), ("MAX_CENT", units.KM_MAX_CENT)):
        assert int(re.search(r"#define FHVAE_KM_%s (\d+)" % name, text).group(1)) == value
    assert units.KM_PIECE == R.PIECE == 256 and units.KM_MAX_ROWS == 2 ** 30 and units.KM_MAX_CENT == 2 ** 20
    for name, value in (("BAD_PTR", units.KM_BAD_PTR), ("BAD_PERM", units.KM_BAD_PERM)):
        assert int(re.search(r"FHVAE_KM_%s = (\d+)" % name, text).group(1)) == value


def test_symbols_exported_and_the_main_header_untouched(lib):
    import hip_binding as hb
    import units

    for name in units.KM_SIGNATURES:
        assert hasattr(lib, name) and name not in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12 and len(hb.SIGNATURES) == 81  # include/fhvae_hip.h is untouched
    header = open(os.path.join(ROOT, "include", "fhvae_hip.h")).read()
    assert "fhvae_km_" not in header and "kmeans" not in header.lower()


def test_assign_errors_before_any_launch(lib):
    keep, p = _aligned()
    ws = lib.fhvae_km_ws_bytes(4, 2, 32)
    fn = lib.fhvae_km_assign
    #       x ldx N  D  cent ldc K ws ws_bytes assign dist stream
    good = [p, 32, 4, 32, p, 32, 2, p, ws, p, p, None]
    for i in (0, 4, 7, 9):
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((3, 8), (3, 136), (3, 40), (3, 0), (1, 28), (5, 16), (2, 0), (2, -1), (6, 0), (6, -3), (8, ws - 1), (8, 0)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i, bad in ((0, p + 4), (4, p + 8), (1, 34), (5, 33), (7, p + 4), (9, p + 2), (10, p + 1)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    assert fn(*_swap(good, 2, (1 << 30) + 1)) == LIMIT and fn(*_swap(good, 6, (1 << 20) + 1)) == LIMIT
    del keep


def test_update_errors_before_any_launch(lib):
    keep, p = _aligned()
    ws = lib.fhvae_km_ws_bytes(4, 2, 32)
    fn = lib.fhvae_km_update
    #       x ldx N  D  perm cl_ptr K dist ws ws_bytes cent ldc count inertia status stream
    good = [p, 32, 4, 32, p, p, 2, p, p, ws, p, 32, p, p, p, None]
    for i in (0, 4, 5, 8, 10, 12, 14):
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((3, 8), (3, 136), (1, 28), (11, 16), (2, 0), (6, 0), (9, ws - 1)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i, bad in ((0, p + 4), (10, p + 4), (1, 34), (4, p + 4), (5, p + 4), (7, p + 2), (8, p + 8), (12, p + 4), (13, p + 4), (14, p + 2)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    assert fn(*_swap(good, 2, (1 << 30) + 1)) == LIMIT and fn(*_swap(good, 6, (1 << 20) + 1)) == LIMIT
    del keep


def test_workspace_is_positive_and_monotone(lib):
    f = lib.fhvae_km_ws_bytes
    for D in (16, 32, 80, 128):
        last = 0
        for N in (1, 2, 255, 256, 257, 1000, 359280, 3592800, 1 << 30):
            v = f(N, 100, D)
            assert v > 0 and v >= last and v % 256 == 0, (N, D)
            last = v
        last = 0
        for K in (1, 2, 63, 64, 65, 1000, 1 << 20):
            v = f(100000, K, D)
            assert v > 0 and v >= last, (K, D)
            last = v
    assert f(1000, 10, 32) < f(1000, 10, 48) < f(1000, 10, 128)
    for bad in ((0, 10, 32), (10, 0, 32), ((1 << 30) + 1, 10, 32), (10, (1 << 20) + 1, 32), (10, 10, 8), (10, 10, 136), (10, 10, 40)):
        assert f(*bad) == 0, bad


# ------------------------------------------------------------------------------------------------------------------ oracle
def test_oracle_update_is_the_two_level_float64_sum():
    # 257 members, one column (the other 15 are zero): 2^24, then 256 ones.  A left-to-right f32 sum loses every one; the float64
    # pieces are exact: (2^24 + 255) + 1
    x = np.zeros((257, 16), dtype=np.float32)
    x[0, 0] = 2.0 ** 24
    x[1:, 0] = 1.0
    f32 = np.float32(0)
    for v in x[:, 0]:
        f32 = np.float32(f32 + v)
    assert f32 == np.float32(2.0 ** 24)
    cent, counts, inertia = R.update(x, np.zeros(257, dtype=np.int32), np.full((1, 16), 7.0, dtype=np.float32))
    want = np.float32((2.0 ** 24 + 256.0) / 257.0)
    assert cent[0, 0] == want != np.float32(f32 / np.float32(257)) and counts.tolist() == [257] and np.all(cent[0, 1:] == 0)
    assert inertia.tolist() == [0.0]
    # 457 members: 2^60 and 255 zeros are the first piece; 200 ones and -2^60 the second, which sums to -(2^60 - 256) (2^60 - 200
    # lies between the float64 neighbours 2^60 - 256 and 2^60 - 128, nearer the first), so the total is 256.  One float64 chain
    # over all members loses the ones against 2^60 and ends at 0
    y = np.zeros((457, 16), dtype=np.float32)
    y[0, 0], y[256:456, 0], y[456, 0] = 2.0 ** 60, 1.0, -(2.0 ** 60)
    flat = 0.0
    for v in y[:, 0]:
        flat += float(v)
    assert flat == 0.0
    labels = np.zeros(457 + 3, dtype=np.int32)
    labels[457:] = 2  # (cluster 1 is empty and keeps its row; cluster 2 has three members)
    rows = np.concatenate([y, np.full((3, 16), 2.0, dtype=np.float32)])
    dist = np.arange(460, dtype=np.float32)
    cent, counts, inertia = R.update(rows, labels, np.full((3, 16), 7.0, dtype=np.float32), dist)
    assert cent[0, 0] == np.float32(256.0 / 457.0) and np.all(cent[1] == 7.0) and np.all(cent[2] == 2.0)
    assert counts.tolist() == [457, 0, 3] and inertia.tolist() == [456 * 457 / 2.0, 0.0, 457.0 + 458.0 + 459.0]


def test_oracle_assign_and_reseed_by_hand():
    x = np.zeros((4, 16), dtype=np.float32)
    x[:, 0] = [0.0, 1.0, 4.0, 10.0]
    cent = np.zeros((3, 16), dtype=np.float32)
    cent[:, 0] = [0.0, 5.0, 5.0]  # (two equal centroids: the first wins)
    labels, d, gap, E = R.assign(x, cent)
    assert labels.tolist() == [0, 0, 1, 1] and d.tolist() == [0.0, 1.0, 1.0, 25.0]
    assert gap.tolist() == [25.0, 15.0, 0.0, 0.0] and E[3] == 2.0 ** -23 * 17 * (100.0 + 25.0)
    counts = np.bincount(labels, minlength=3)
    assert R.reseed(labels, d, counts) == 1 and labels.tolist() == [0, 0, 1, 2]  # (the farthest row goes to the empty cluster)
    d2 = np.array([1.0, 3.0, 3.0, 0.0])
    l2 = np.zeros(4, dtype=np.int32)
    assert R.reseed(l2, d2, np.array([4, 0, 0])) == 2 and l2.tolist() == [0, 1, 2, 0]  # (equal dist: the smaller row first)


# ----------------------------------------------------------------------------------------------------------------- metrics
def _frames_of(table):
    labels, phones = [], []
    for u, row in enumerate(table):
        for p, c in enumerate(row):
            labels += [u] * c
            phones += [p] * c
    return np.asarray(labels, dtype=np.int32), np.asarray(phones, dtype=np.int32)


def test_unit_quality_on_a_table_done_by_hand():
    import units

    labels, phones = _frames_of([[4, 1, 0], [0, 3, 1], [1, 0, 2]])
    labels, phones = np.concatenate([labels, [0, 2]]).astype(np.int32), np.concatenate([phones, [-1, -1]]).astype(np.int32)
    # n = 12, unit sums (5, 4, 3), phone sums (5, 4, 3)
    mi = (4 / 12 * math.log(4 * 12 / 25) + 1 / 12 * math.log(1 * 12 / 20) + 3 / 12 * math.log(3 * 12 / 16) + 1 / 12 * math.log(1 * 12 / 12)
          + 1 / 12 * math.log(1 * 12 / 15) + 2 / 12 * math.log(2 * 12 / 9))
    hp = -(5 / 12 * math.log(5 / 12) + 4 / 12 * math.log(4 / 12) + 3 / 12 * math.log(3 / 12))
    for f in (units.unit_quality, R.unit_quality):
        q = f(labels, phones, 3)
        assert q["labelled_frames"] == 12 and q["cluster_purity"] == pytest.approx(9 / 12, abs=1e-15)
        assert q["phone_purity"] == pytest.approx(9 / 12, abs=1e-15) and q["pnmi"] == pytest.approx(mi / hp, abs=1e-14)
        assert 0.0 < q["pnmi"] < 1.0
        # a perfect clustering (units are a renaming of the phones): all three are 1
        q = f(*_frames_of([[0, 5, 0], [0, 0, 2], [7, 0, 0]]), 3)
        assert q["cluster_purity"] == 1.0 and q["phone_purity"] == 1.0 and q["pnmi"] == pytest.approx(1.0, abs=1e-15)
        # one cluster: it tells nothing about the phone
        q = f(*_frames_of([[6, 3, 1]]), 1)
        assert q["pnmi"] == 0.0 and q["cluster_purity"] == pytest.approx(0.6, abs=1e-15) and q["phone_purity"] == 1.0
        # one phone: H(phone) = 0
        q = f(*_frames_of([[6], [3]]), 2)
        assert q["pnmi"] == 0.0 and q["cluster_purity"] == 1.0 and q["phone_purity"] == pytest.approx(6 / 9, abs=1e-15)
        q = f(np.zeros(3, np.int32), np.full(3, -1, np.int32), 2)
        assert q == {"cluster_purity": 0.0, "phone_purity": 0.0, "pnmi": 0.0, "labelled_frames": 0}
    # an empty unit and an empty phone column change nothing
    labels, phones = _frames_of([[4, 1, 0], [0, 3, 1], [1, 0, 2]])
    assert units.unit_quality(labels, phones, 5, n_phones=6)["pnmi"] == pytest.approx(mi / hp, abs=1e-14)


def test_bitrate_of_a_two_symbol_sequence():
    import units

    for f in (units.bitrate, R.bitrate):
        # 4 symbols, 1 bit each, in 0.04 s; collapsed: 2 symbols of 1 bit over the same 0.04 s
        assert f([[0, 0, 1, 1]], 0.010) == {"bitrate": 100.0, "bitrate_collapsed": 50.0}
        # two utterances share one distribution: (3/4, 1/4) over 8 symbols in 0.16 s; collapsed (5, 2) and (5, 2, 5): (3/5, 2/5)
        h = -(0.75 * math.log2(0.75) + 0.25 * math.log2(0.25))
        hc = -(0.6 * math.log2(0.6) + 0.4 * math.log2(0.4))
        got = f([np.array([5, 5, 5, 2]), np.array([5, 5, 2, 5])], 0.020)
        assert got["bitrate"] == pytest.approx(8 * h / 0.16, rel=1e-14) and got["bitrate_collapsed"] == pytest.approx(5 * hc / 0.16, rel=1e-14)
        assert f([[3, 3, 3]], 0.010) == {"bitrate": 0.0, "bitrate_collapsed": 0.0}
    assert units.collapse([1, 1, 2, 2, 2, 1, 3, 3]).tolist() == [1, 2, 1, 3] and units.collapse([]).shape == (0,)


# ------------------------------------------------------------------------------------------------------------------ phones
def test_frame_phones():
    import units

    items = [("u1", 0.10, 0.15, "aa", "b", "k", "s1"),   # frames 10..15: the frame exactly at the onset belongs to the token
             ("zz", 0.00, 0.05, "zh", "b", "k", "s1"),   # unknown utterance: labels nothing, names no phone
             ("u1", 0.14, 0.20, "iy", "b", "k", "s1"),   # frames 14..20: 14 and 15 stay "aa"
             ("u2", 0.00, 0.29, "aa", "b", "k", "s2"),   # a token of 30 frames: no cap on the length
             ("u2", 0.101, 0.109, "s", "b", "k", "s2"),  # no frame
             ("u2", 0.05, 0.06, "s", "b", "k", "s2")]    # wholly covered already
    phones, names, overlaps = units.frame_phones(items, ["u1", "u2"], [50, 30])
    assert phones.dtype == np.int32 and phones.shape == (80,) and names == ["aa", "iy", "s"] and overlaps == 2 + 2
    want = np.full(80, -1)
    want[10:16], want[16:21], want[50:80] = 0, 1, 0
    assert phones.tolist() == want.tolist()
    # Kaldi's snip-edges frames of 25 ms are centred at 12.5 ms + 10 ms f: [0.10, 0.15] holds frames 9..13
    phones, names, overlaps = units.frame_phones(items[:1], ["u0", "u1"], [7, 50], 0.010, 0.0125)
    assert np.nonzero(phones >= 0)[0].tolist() == [7 + 9, 7 + 10, 7 + 11, 7 + 12, 7 + 13] and names == ["aa"] and overlaps == 0
    phones, names, overlaps = units.frame_phones([], ["u1"], [5])
    assert phones.tolist() == [-1] * 5 and names == [] and overlaps == 0
    with pytest.raises(ValueError):
        units.frame_phones(items, ["u1"], [50], frame_shift=0.0)


def test_units_text_round_trip(tmp_path):
    import units

    keys = ["s01-1-0000", "s01-1-0001", "b"]
    seqs = [np.array([3, 3, 0, 12], dtype=np.int32), np.array([7], dtype=np.int32), np.arange(300, dtype=np.int32)]
    path = str(tmp_path / "units.txt")
    units.write_units(path, keys, seqs)
    lines = open(path).read().splitlines()
    assert lines[0] == "s01-1-0000 3 3 0 12" and lines[1] == "s01-1-0001 7" and len(lines) == 3
    got_keys, got = units.read_units(path)
    assert got_keys == keys and all(g.dtype == np.int32 and g.tolist() == s.tolist() for g, s in zip(got, seqs))
    with pytest.raises(ValueError):
        units.write_units(path, keys[:2], seqs)
    (tmp_path / "bad.txt").write_text("a 1 2\nb 1 x\n")
    with pytest.raises(ValueError, match="line 2"):
        units.read_units(str(tmp_path / "bad.txt"))


# --------------------------------------------------------------------------------------------------------------------- CLI
def test_command_line_argument_errors(tmp_path, capsys):
    import discover_units as DU
    import eval_model as EM

    base = ["--checkpoint", str(tmp_path / "c.tar"), "--feat-scp", str(tmp_path / "f.scp"), "--len-scp", str(tmp_path / "l.scp"),
            "--out", str(tmp_path / "o")]
    for extra in ([], ["--k", "4", "--codebook", str(tmp_path / "c.npy")], ["--k", "0"], ["--k", "4", "--iters", "0"]):
        with pytest.raises(SystemExit) as e:
            DU.main(base + extra)
        assert e.value.code == 2, extra
    with pytest.raises(SystemExit) as e:
        EM.parse_args(["--checkpoint", "c.tar", "--out", str(tmp_path / "o"), "--units", "4"])
    assert e.value.code == 2 and "--feat-scp" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        EM.parse_args(["--checkpoint", "c.tar", "--out", str(tmp_path / "o"), "--feat-scp", "f.scp", "--units", "0"])
    assert e.value.code == 2
    args = EM.parse_args(["--checkpoint", "c.tar", "--out", "o"])
    assert args.units is None and args.units_on == ["z1", "feats"] and args.units_iters == 100 and args.units_seed == 0
