"""ABX without a GPU: the item format and its errors, the mapping of times to frames at its boundaries, max_per_cell,
abx_scores against the literal triple loop of abx_ref, tools/timit_items.py on a generated tree, the entry point's export, its
argument errors (they return before any launch) and ABX_SIGNATURES against include/fhvae_abx.h."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import abx_ref as R
import ext_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import abx

    return abx.load_library()


# ------------------------------------------------------------------------------------------------------------------- items
def test_read_items_and_its_errors(tmp_path):
    import abx

    path = tmp_path / "a.item"
    path.write_text(abx.ITEM_HEADER + "\nu1 0.10 0.25 aa b k spk1\n\nu2 1 1.5 iy h# t spk2\n")
    assert abx.read_items(str(path)) == [("u1", 0.10, 0.25, "aa", "b", "k", "spk1"), ("u2", 1.0, 1.5, "iy", "h#", "t", "spk2")]
    abx.write_items(str(tmp_path / "b.item"), abx.read_items(str(path)))
    assert abx.read_items(str(tmp_path / "b.item")) == abx.read_items(str(path))
    for body, line in (("u1 0.1 0.2 aa b k\n", 2), ("u1 0.1 0.2 aa b k s\nu1 x 0.2 aa b k s\n", 3), ("u1 0.3 0.2 aa b k s\n", 2),
                       ("u1 0.1 0.2 aa b k s extra\n", 2), ("u1 0.1 nan aa b k s\n", 2)):
        path.write_text(abx.ITEM_HEADER + "\n" + body)
        with pytest.raises(ValueError, match="line %d" % line):
            abx.read_items(str(path))


def test_frame_mapping_at_the_boundaries():
    import abx

    # a frame exactly at the onset and one exactly at the offset belong to the token: 0.10 / 0.01 is 10.000000000000002 in binary
    assert abx.frame_range(0.10, 0.15, 100) == (10, 6)
    assert abx.frame_range(0.101, 0.149, 100) == (11, 4)
    assert abx.frame_range(0.29, 0.30, 100) == (29, 2)
    # Kaldi's snip-edges frames of 25 ms are centred at 12.5 ms + 10 ms f
    assert abx.frame_range(0.10, 0.15, 100, 0.010, 0.0125) == (9, 5)
    assert abx.frame_range(0.0125, 0.0125, 100, 0.010, 0.0125) == (0, 1)
    # clipped to the utterance: an offset past its end, an onset before its first frame
    assert abx.frame_range(0.95, 1.20, 100) == (95, 5)
    assert abx.frame_range(0.0, 0.02, 100, 0.010, 0.0125) == (0, 1)
    # no frame: between two frames, or wholly past the end
    assert abx.frame_range(0.101, 0.109, 100)[1] == 0
    assert abx.frame_range(1.00, 1.20, 100)[1] == 0


def test_tokens_from_items_drops_and_counts():
    import abx

    items = [("u1", 0.00, 0.05, "aa", "b", "k", "s1"),     # frames 0..5
             ("zz", 0.00, 0.05, "aa", "b", "k", "s1"),     # unknown utterance
             ("u2", 0.101, 0.109, "aa", "b", "k", "s2"),   # no frame
             ("u2", 0.00, 0.64, "iy", "b", "k", "s2"),     # 65 frames: too long
             ("u2", 0.00, 0.63, "iy", "b", "k", "s2"),     # 64 frames
             ("u2", 0.95, 2.00, "iy", "d", "k", "s2")]     # clipped to frames 95..99
    t = abx.tokens_from_items(items, ["u1", "u2"], [50, 100], max_per_cell=0)
    assert t["dropped"] == {"unknown_utterance": 1, "no_frames": 1, "too_long": 1, "over_cell_cap": 0}
    assert t["start"].tolist() == [0, 50, 145] and t["len"].tolist() == [6, 64, 5] and t["utt"].tolist() == [0, 1, 1]
    assert t["start"].dtype == np.int64 and t["len"].dtype == np.int32
    assert t["phones"] == ["aa", "iy"] and t["contexts"] == [("b", "k"), ("d", "k")] and t["speakers"] == ["s1", "s2"]
    assert t["phone"].tolist() == [0, 1, 1] and t["ctx"].tolist() == [0, 0, 1] and t["spk"].tolist() == [0, 1, 1]
    t = abx.tokens_from_items(items, ["u1", "u2"], [50, 100], max_len=5, max_per_cell=0)
    assert t["len"].tolist() == [5] and t["dropped"]["too_long"] == 3
    with pytest.raises(ValueError):
        abx.tokens_from_items(items, ["u1", "u2"], [50, 100], max_len=65)
    empty = abx.tokens_from_items([], ["u1"], [50])
    assert empty["start"].shape == (0,) and empty["phones"] == []


def test_max_per_cell_keeps_the_first_of_every_cell_in_file_order():
    import abx

    items = []
    for k in range(5):
        items.append(("u1", 0.1 * k, 0.1 * k + 0.03, "aa", "b", "k", "s1"))
        items.append(("u1", 0.1 * k + 0.04, 0.1 * k + 0.06, "aa", "b", "k", "s2"))  # another speaker: another cell
        items.append(("u1", 0.1 * k + 0.07, 0.1 * k + 0.09, "aa", "b", "t", "s1"))  # another context
    t = abx.tokens_from_items(items, ["u1"], [60], max_per_cell=2)
    assert t["start"].tolist() == [0, 4, 7, 10, 14, 17] and t["dropped"]["over_cell_cap"] == 9
    assert len(abx.tokens_from_items(items, ["u1"], [60], max_per_cell=0)["start"]) == 15
    assert len(abx.tokens_from_items(items, ["u1"], [60])["start"]) == 15  # (the default cap is 20)


# ------------------------------------------------------------------------------------------------------------------ scores
def _score_case():
    """40 tokens, 3 phones, 2 contexts, 3 speakers, integer distances (so equal distances occur).  Speaker 2 appears in context
    0 only; (phone 2, context 1, speaker 0) has a single token: no A != X there."""
    rng = np.random.default_rng(5)
    phone, ctx, spk = rng.integers(0, 3, 40), rng.integers(0, 2, 40), rng.integers(0, 2, 40)
    spk[:6], ctx[:6] = 2, 0
    lone = (phone == 2) & (ctx == 1) & (spk == 0)
    phone[np.nonzero(lone)[0][1:]] = 1
    d = rng.integers(1, 6, (40, 40)).astype(np.float32)
    d = np.triu(d, 1) + np.triu(d, 1).T
    tokens = {"phone": phone, "ctx": ctx, "spk": spk, "phones": ["p0", "p1", "p2"], "contexts": [("a", "b"), ("c", "d")],
              "speakers": ["s0", "s1", "s2"], "dropped": {"no_frames": 3}}
    blocks = []
    for c in (1, 0):  # (any order of the blocks)
        idx = np.nonzero(ctx == c)[0]
        blocks.append((c, idx, d[np.ix_(idx, idx)]))
    return tokens, blocks, d


def test_abx_scores_equal_the_triple_loop():
    import abx

    tokens, blocks, d = _score_case()
    phone, ctx, spk = tokens["phone"], tokens["ctx"], tokens["spk"]
    assert ((phone == 2) & (ctx == 1) & (spk == 0)).sum() == 1 and not ((spk == 2) & (ctx == 1)).any()
    want = R.abx_triples(lambda a, b: d[a, b], phone, ctx, spk)
    got = abx.abx_scores(blocks, tokens)
    assert want["eq_within"] > 0 and want["eq_across"] > 0  # ties are scored 1/2
    for task in ("within", "across"):
        for key in ("cells_", "triples_", "gt_", "eq_"):
            assert got[key + task] == want[key + task] > 0, key + task
        assert abs(got[task] - want[task]) <= 1e-12
    assert got["tokens"] == 40 and got["dropped"] == {"no_frames": 3}
    assert got["by_pair_within"].shape == (3, 3) and np.isnan(np.diag(got["by_pair_within"])).all()


def test_abx_scores_on_cases_done_by_hand():
    import abx

    # one context, one speaker: A, X of phone 0 at distance 1; B of phone 1 at distance 1 from one and 3 from the other
    tokens = {"phone": np.array([0, 0, 1]), "ctx": np.zeros(3, int), "spk": np.zeros(3, int), "phones": ["p", "q"]}
    block = np.array([[0, 1, 1], [1, 0, 3], [1, 3, 0]], dtype=np.float32)
    got = abx.abx_scores([(0, np.arange(3), block)], tokens)
    # (p, q): X = 0: d(A=1, X) = 1 = d(B, X) = 1 -> 1/2;  X = 1: d(A=0, X) = 1 < 3 -> 0;  cell = 1/4.  (q, p) has no A != X
    assert got["within"] == 0.25 and got["cells_within"] == 1 and got["triples_within"] == 2 and got["eq_within"] == 1
    assert np.isnan(got["across"]) and got["cells_across"] == 0 and got["triples_across"] == 0
    # no token at all
    none = abx.abx_scores([], {"phone": np.zeros(0, int), "spk": np.zeros(0, int), "phones": []})
    assert np.isnan(none["within"]) and none["tokens"] == 0


def test_write_by_pair(tmp_path):
    import abx

    tokens, blocks, _ = _score_case()
    res = abx.abx_scores(blocks, tokens)
    abx.write_by_pair(str(tmp_path / "p.tsv"), res, tokens["phones"])
    lines = (tmp_path / "p.tsv").read_text().splitlines()
    assert lines[0].split("\t") == ["phone", "other", "within", "across"] and len(lines) == 1 + 6
    assert all(len(ln.split("\t")) == 4 for ln in lines)


# ------------------------------------------------------------------------------------------------------------------- TIMIT
def test_timit_items_on_a_generated_tree(tmp_path, capsys):
    import abx

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import timit_items as TI
    finally:
        sys.path.pop(0)
    a, b = tmp_path / "TRAIN" / "DR1" / "FCJF0", tmp_path / "TEST" / "DR2" / "MABC0"
    os.makedirs(a), os.makedirs(b)
    (a / "SA1.PHN").write_text("0 3050 h#\n3050 4559 sh\n4559 5723 ix\n5723 6642 hv\n6642 8772 h#\n")
    (a / "SA1.WAV").write_text("not read")
    (b / "SI648.PHN").write_text("0 1600 h#\n1600 3200 d\n3200 4000 h#\n4000 4800 ow\n4800 8000 n\n8000 9600 h#\n")
    assert TI.main([str(tmp_path), str(tmp_path / "t.item")]) == 0
    assert "6 items of 2 utterances" in capsys.readouterr().out
    items = abx.read_items(str(tmp_path / "t.item"))
    # sorted walk: TEST before TRAIN.  h# and each file's first and last phone are no tokens; h# is a context
    assert [it[:1] + it[3:] for it in items] == [("mabc0_SI648", "d", "h#", "h#", "mabc0"), ("mabc0_SI648", "ow", "h#", "n", "mabc0"),
                                                 ("mabc0_SI648", "n", "ow", "h#", "mabc0"), ("fcjf0_SA1", "sh", "h#", "ix", "fcjf0"),
                                                 ("fcjf0_SA1", "ix", "sh", "hv", "fcjf0"), ("fcjf0_SA1", "hv", "ix", "h#", "fcjf0")]
    times = [(1600, 3200), (4000, 4800), (4800, 8000), (3050, 4559), (4559, 5723), (5723, 6642)]
    for it, (s0, s1) in zip(items, times):
        assert it[1] == pytest.approx(s0 / 16000, abs=1e-6) and it[2] == pytest.approx(s1 / 16000, abs=1e-6)
    (b / "SI648.PHN").write_text("0 1600 h#\n1600 d\n")
    assert TI.main([str(tmp_path), str(tmp_path / "t.item")]) == 1
    assert "SI648.PHN line 2" in capsys.readouterr().err


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_signature_matches_the_header():
    import abx
    import hip_binding as hb

    text = ext_abi.header_text("fhvae_abx.h")
    found = ext_abi.declared("fhvae_abx.h", "fhvae_abx_")
    assert found == abx.ABX_SIGNATURES and sorted(found) == ["fhvae_abx_dtw"]
    assert not set(found) & set(hb.SIGNATURES)
    for name, value in (("MAX_DIM", abx.ABX_MAX_DIM), ("MAX_LEN", abx.ABX_MAX_LEN)):
        assert int(re.search(r"#define FHVAE_ABX_%s (\d+)" % name, text).group(1)) == value
    for name, value in (("ANGULAR", abx.ABX_ANGULAR), ("COSINE", abx.ABX_COSINE), ("BAD_TOKEN", abx.ABX_BAD_TOKEN),
                        ("BAD_PTR", abx.ABX_BAD_PTR)):
        assert int(re.search(r"FHVAE_ABX_%s = (\d+)" % name, text).group(1)) == value


def test_symbol_exported_and_errors_before_any_launch(lib):
    import abx
    import hip_binding as hb

    assert hasattr(lib, "fhvae_abx_dtw") and "fhvae_abx_dtw" not in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12 and len(hb.SIGNATURES) == 81  # include/fhvae_hip.h is untouched
    header = open(os.path.join(ROOT, "include", "fhvae_hip.h")).read()
    assert "abx" not in header.lower()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    NULL, SHAPE, LIMIT = -1, -2, -5
    fn = lib.fhvae_abx_dtw
    #       feats nfr D  start len N maxlen grp out pair G  npairs nout metric out status stream
    good = [p, 64, 8, p, p, 2, 64, p, p, p, 1, 1, 4, 0, p, p, None]

    def swap(i, v):
        return [v if j == i else a for j, a in enumerate(good)]

    for i in (0, 3, 4, 7, 8, 9, 14, 15):
        assert fn(*swap(i, None)) == NULL, i
    for i, bad in ((1, -1), (2, 0), (2, -3), (5, -1), (6, 0), (6, -64), (10, -1), (11, -1), (12, -1), (13, 2), (13, -1)):
        assert fn(*swap(i, bad)) == SHAPE, (i, bad)
    assert fn(*swap(2, abx.ABX_MAX_DIM + 1)) == LIMIT and fn(*swap(6, abx.ABX_MAX_LEN + 1)) == LIMIT
    for i in (5, 10, 11):
        assert fn(*swap(i, 1 << 31)) == LIMIT, i
    assert fn(*swap(5, 0)) == 0 and fn(*swap(10, 0)) == 0  # N == 0 or G == 0: nothing to do, nothing launched
