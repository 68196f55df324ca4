"""Query-by-example search without a GPU: QBE_SIGNATURES against include/fhvae_qbe.h, the entry point's export and its argument
errors (they return before any launch), queries_from_items' drops and caps, rank_metrics against the literal loop of qbe_ref and
on cases done by hand, tools/timit_items.py --tier wrd on a generated tree, and the oracle against the ABX oracle."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import abx_ref
import qbe_ref as R
import ext_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import qbe

    return qbe.load_library()


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_signature_matches_the_header():
    import abx
    import hip_binding as hb
    import qbe

    text = ext_abi.header_text("fhvae_qbe.h")
    found = ext_abi.declared("fhvae_qbe.h", "fhvae_qbe_")
    assert found == qbe.QBE_SIGNATURES and sorted(found) == ["fhvae_qbe_sdtw"]
    assert not set(found) & set(hb.SIGNATURES) and not set(found) & set(abx.ABX_SIGNATURES)
    for name, value in (("MAX_DIM", qbe.QBE_MAX_DIM), ("MAX_QLEN", qbe.QBE_MAX_QLEN)):
        assert int(re.search(r"#define FHVAE_QBE_%s (\d+)" % name, text).group(1)) == value
    for name, value in (("ANGULAR", qbe.QBE_ANGULAR), ("COSINE", qbe.QBE_COSINE), ("BAD_QUERY", qbe.QBE_BAD_QUERY),
                        ("BAD_PTR", qbe.QBE_BAD_PTR)):
        assert int(re.search(r"FHVAE_QBE_%s = (\d+)" % name, text).group(1)) == value
    assert qbe.METRICS == abx.METRICS and qbe.QBE_MAX_DIM == abx.ABX_MAX_DIM  # the frame cost is ABX's


def test_symbol_exported_and_errors_before_any_launch(lib):
    import hip_binding as hb
    import qbe

    assert hasattr(lib, "fhvae_qbe_sdtw") and "fhvae_qbe_sdtw" not in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12 and len(hb.SIGNATURES) == 81  # include/fhvae_hip.h is untouched
    header = open(os.path.join(ROOT, "include", "fhvae_hip.h")).read()
    assert "qbe" not in header.lower()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    NULL, SHAPE, LIMIT = -1, -2, -5
    fn = lib.fhvae_qbe_sdtw
    #       qfeats nqf feats nfr D qstart qlen Q maxq utt U metric cost start end ecost estart status stream
    good = [p, 8, p, 8, 8, p, p, 2, 64, p, 3, 0, p, p, p, p, p, p, None]

    def swap(i, v):
        return [v if j == i else a for j, a in enumerate(good)]

    for i in (0, 2, 5, 6, 9, 12, 13, 14, 17):
        assert fn(*swap(i, None)) == NULL, i
    for i, bad in ((1, -1), (3, -1), (4, 0), (4, -3), (7, -1), (8, 0), (8, -64), (10, -1), (11, 2), (11, -1)):
        assert fn(*swap(i, bad)) == SHAPE, (i, bad)
    assert fn(*swap(4, qbe.QBE_MAX_DIM + 1)) == LIMIT and fn(*swap(8, qbe.QBE_MAX_QLEN + 1)) == LIMIT
    for i in (7, 10):
        assert fn(*swap(i, 1 << 31)) == LIMIT, i
    big = list(good)
    big[7], big[10] = 1 << 16, 1 << 15  # Q * U = 2^31
    assert fn(*big) == LIMIT
    big[3] = 1 << 60  # Q * n_frames past 2^63 with a profile asked for
    big[10] = 1
    assert fn(*big) == LIMIT
    assert fn(*swap(7, 0)) == 0 and fn(*swap(10, 0)) == 0  # Q == 0 or U == 0: nothing to do, nothing launched


# ------------------------------------------------------------------------------------------------------------------- items
def test_queries_from_items_drops_and_caps():
    import qbe

    items = [("u1", 0.00, 0.05, "cat", "-", "-", "s1"),     # frames 0..5
             ("zz", 0.00, 0.05, "cat", "-", "-", "s1"),     # unknown utterance
             ("u2", 0.101, 0.109, "cat", "-", "-", "s2"),   # no frame
             ("u2", 0.00, 0.64, "dog", "-", "-", "s2"),     # 65 frames: too long
             ("u2", 0.00, 0.63, "dog", "-", "-", "s2"),     # 64 frames
             ("u2", 0.95, 2.00, "cat", "-", "-", "s2"),     # clipped to frames 95..99
             ("u2", 0.20, 0.29, "cat", "-", "-", "s2"),     # the third kept cat
             ("u1", 0.10, 0.12, "dog", "-", "-", "s1")]
    q = qbe.queries_from_items(items, ["u1", "u2"], [50, 100], max_per_term=0)
    assert q["dropped"] == {"unknown_utterance": 1, "no_frames": 1, "too_long": 1, "over_term_cap": 0}
    assert q["start"].tolist() == [0, 50, 145, 70, 10] and q["len"].tolist() == [6, 64, 5, 10, 3]
    assert q["utt"].tolist() == [0, 1, 1, 1, 0] and q["first"].tolist() == [0, 0, 95, 20, 10]
    assert q["start"].dtype == np.int64 and q["len"].dtype == np.int32
    assert q["terms"] == ["cat", "dog"] and q["term"].tolist() == [0, 1, 0, 0, 1]
    assert q["id"] == ["cat_0", "dog_0", "cat_1", "cat_2", "dog_1"]
    q = qbe.queries_from_items(items, ["u1", "u2"], [50, 100], max_per_term=2)  # the first two of every term in file order
    assert q["id"] == ["cat_0", "dog_0", "cat_1", "dog_1"] and q["dropped"]["over_term_cap"] == 1
    assert len(qbe.queries_from_items(items, ["u1", "u2"], [50, 100])["start"]) == 5  # (the default cap is 5)
    q = qbe.queries_from_items(items, ["u1", "u2"], [50, 100], max_len=5, max_per_term=0)
    assert q["len"].tolist() == [5, 3] and q["dropped"]["too_long"] == 4
    for bad in ({"max_len": 65}, {"max_len": 0}, {"max_per_term": -1}, {"frame_shift": 0.0}):
        with pytest.raises(ValueError):
            qbe.queries_from_items(items, ["u1", "u2"], [50, 100], **bad)
    empty = qbe.queries_from_items([], ["u1"], [50])
    assert empty["start"].shape == (0,) and empty["terms"] == [] and empty["id"] == []
    # the truth keeps tokens of any length and drops what has no utterance or no frame
    t = qbe.truth_from_items(items, ["u1", "u2"], [50, 100])
    assert t["utt"].tolist() == [0, 1, 1, 1, 1, 0] and t["first"].tolist() == [0, 0, 0, 95, 20, 10]
    assert t["last"].tolist() == [5, 64, 63, 99, 29, 12] and t["term"] == ["cat", "dog", "dog", "cat", "cat", "dog"]


# ------------------------------------------------------------------------------------------------------------------ scores
def _metrics_both(cost, bs, be, queries, truth, same_corpus=True):
    import qbe

    got = qbe.rank_metrics(cost, bs, be, queries, truth, same_corpus)
    q_term = [queries["terms"][t] for t in queries["term"]]
    rows = list(zip(truth["utt"].tolist(), truth["first"].tolist(), truth["last"].tolist(), truth["term"]))
    want = R.rank_metrics(cost, bs, be, q_term, queries["utt"].tolist(), rows, same_corpus)
    assert set(got) == set(want) == {"map", "p_at_n", "p_at_10", "located", "queries", "no_target"}
    for k in want:
        if isinstance(want[k], float):
            assert abs(got[k] - want[k]) <= 1e-12, k
        else:
            assert got[k] == want[k], k
    return got


def _truth(rows):
    return {"utt": np.array([r[0] for r in rows], dtype=np.int64), "first": np.array([r[1] for r in rows], dtype=np.int64),
            "last": np.array([r[2] for r in rows], dtype=np.int64), "term": [r[3] for r in rows]}


def test_rank_metrics_equal_the_literal_loop():
    rng = np.random.default_rng(11)
    Q, U = 30, 25
    terms = ["t%d" % k for k in range(6)]
    queries = {"term": rng.integers(0, 6, Q), "terms": terms, "utt": rng.integers(0, U, Q)}
    rows = [(int(rng.integers(0, U)), int(f), int(f + rng.integers(3, 40)), terms[int(rng.integers(0, 5))])  # t5 has no token
            for f in rng.integers(0, 200, 40)]
    cost = rng.integers(1, 8, (Q, U)).astype(np.float32) / 8  # few values: equal costs are the rule
    be = rng.integers(0, 240, (Q, U)).astype(np.int32)
    bs = (be - rng.integers(0, 30, (Q, U))).clip(0).astype(np.int32)
    cost[3, 7], bs[3, 7], be[3, 7] = np.inf, -1, -1  # an empty utterance
    for same in (True, False):
        got = _metrics_both(cost, bs, be, queries, _truth(rows), same)
        assert got["no_target"] >= int((queries["term"] == 5).sum()) > 0 and got["queries"] + got["no_target"] == Q
        assert 0 < got["map"] < 1 and 0 < got["located"] < 1


def test_rank_metrics_on_cases_done_by_hand():
    import qbe

    queries = {"term": np.array([0, 0, 1]), "terms": ["cat", "dog"], "utt": np.array([0, 1, 2])}
    truth = _truth([(0, 10, 19, "cat"), (1, 40, 49, "cat"), (3, 5, 14, "cat"), (2, 0, 9, "dog")])
    #               u0   u1   u2   u3   u4
    cost = np.array([[.0, .3, .3, .3, .1],    # cat from u0: u0 is out; u4 first, then u1, u2, u3 tie -> by index: ranks 2 and 4
                     [.5, .0, .2, .1, .4],    # cat from u1: u3 first, u0 last
                     [.1, .2, .0, .3, .4]],   # dog from u2: its only token is its own utterance
                    dtype=np.float32)
    bs = np.array([[0, 44, 0, 0, 0], [12, 0, 0, 11, 0], [0, 0, 0, 0, 0]], dtype=np.int32)
    be = np.array([[5, 53, 5, 5, 5], [25, 5, 5, 30, 5], [5, 5, 5, 5, 5]], dtype=np.int32)
    got = _metrics_both(cost, bs, be, queries, truth)
    assert got["queries"] == 2 and got["no_target"] == 1
    # query 0: relevant u1 (rank 2), u3 (rank 4): AP = (1/2 + 2/4) / 2 = 1/2, P@2 = 1/2; 4 candidates: P@10 = 2/4
    # query 1: relevant u0 (rank 4), u3 (rank 1): AP = (1 + 2/4) / 2 = 3/4, P@2 = 1/2, P@10 = 2/4
    assert got["map"] == pytest.approx(0.625, abs=1e-15) and got["p_at_n"] == 0.5 and got["p_at_10"] == 0.5
    # located: q0/u1 [44, 53] on [40, 49]: 6 of 10 frames; q0/u3 [0, 5] on [5, 14]: 1 of 6, no.
    #          q1/u0 [12, 25] on [10, 19]: 8 of 10; q1/u3 [11, 30] on [5, 14]: 4 of 10, no
    assert got["located"] == 0.5
    # queries cut from another corpus: nothing is taken out, the dog query finds its own utterance first
    other = _metrics_both(cost, bs, be, queries, truth, same_corpus=False)
    assert other["queries"] == 3 and other["no_target"] == 0
    # no query at all, and queries that all lack a target: None, not a division by zero
    for q, c in (({"term": np.zeros(0, int), "terms": [], "utt": np.zeros(0, int)}, np.zeros((0, 5), np.float32)),
                 ({"term": np.array([1]), "terms": ["cat", "dog"], "utt": np.array([2])}, cost[2:])):
        none = qbe.rank_metrics(c, bs[:len(c)], be[:len(c)], q, truth)
        assert none["map"] is None and none["p_at_n"] is None and none["p_at_10"] is None and none["located"] is None
        assert none["queries"] == 0 and none["no_target"] == len(c)
    hits = qbe.top_hits(cost, bs, be, queries, 2)
    assert [[h[:2] for h in row] for row in hits] == [[(1, 4), (2, 1)], [(1, 3), (2, 2)], [(1, 0), (2, 1)]]
    assert hits[0][1] == (2, 1, 44, 53, pytest.approx(0.3, abs=1e-7))


# ------------------------------------------------------------------------------------------------------------------- TIMIT
def test_timit_word_items_on_a_generated_tree(tmp_path, capsys):
    import abx
    import qbe

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import timit_items as TI
    finally:
        sys.path.pop(0)
    a, b = tmp_path / "TRAIN" / "DR1" / "FCJF0", tmp_path / "TEST" / "DR2" / "MABC0"
    os.makedirs(a), os.makedirs(b)
    (a / "SA1.WRD").write_text("3050 5723 she\n5723 10337 had\n10337 12640 she\n")
    (a / "SA1.PHN").write_text("0 3050 h#\n3050 4559 sh\n4559 5723 ix\n5723 6642 hv\n6642 8772 h#\n")
    (b / "SI648.wrd").write_text("1600 8000 had\n")
    assert TI.main([str(tmp_path), str(tmp_path / "w.item"), "--tier", "wrd"]) == 0
    assert "4 items of 2 utterances" in capsys.readouterr().out
    items = abx.read_items(str(tmp_path / "w.item"))
    assert [it[:1] + it[3:] for it in items] == [("mabc0_SI648", "had", "-", "-", "mabc0"), ("fcjf0_SA1", "she", "-", "-", "fcjf0"),
                                                 ("fcjf0_SA1", "had", "-", "-", "fcjf0"), ("fcjf0_SA1", "she", "-", "-", "fcjf0")]
    for it, (s0, s1) in zip(items, [(1600, 8000), (3050, 5723), (5723, 10337), (10337, 12640)]):
        assert it[1] == pytest.approx(s0 / 16000, abs=1e-6) and it[2] == pytest.approx(s1 / 16000, abs=1e-6)
    q = qbe.queries_from_items(items, ["fcjf0_SA1", "mabc0_SI648"], [100, 60])
    assert q["id"] == ["had_0", "she_0", "had_1", "she_1"] and q["utt"].tolist() == [1, 0, 0, 0]
    # the phone tier is what it was: the .WRD files are not read
    assert TI.main([str(tmp_path), str(tmp_path / "p.item")]) == 0
    assert [it[3] for it in abx.read_items(str(tmp_path / "p.item"))] == ["sh", "ix", "hv"]
    (b / "SI648.wrd").write_text("1600 had\n")
    assert TI.main([str(tmp_path), str(tmp_path / "w.item"), "--tier", "wrd"]) == 1
    assert "SI648.wrd line 1" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------------------------ oracle
@pytest.mark.parametrize("metric", ["angular", "cosine"])
@pytest.mark.parametrize("n,m,D", [(5, 40, 8), (17, 90, 32), (30, 70, 3)])
def test_oracle_against_the_abx_oracle(n, m, D, metric):
    """e[j] is the ABX distance between the query and the frames s[j] .. j it was aligned to, bit for bit: the subsequence
    recursion and the whole-token recursion are the same arithmetic once the start is known."""
    rng = np.random.default_rng(100 * n + D)
    q, u = rng.standard_normal((n, D)).astype(np.float32), rng.standard_normal((m, D)).astype(np.float32)
    e, s, gap = R.sdtw(q, u, metric)
    assert e.dtype == np.float32 and e.shape == s.shape == gap.shape == (m,)
    assert np.all(s >= 0) and np.all(s <= np.arange(m)) and np.all(np.diff(s) >= 0)  # (paths do not cross)
    for j in range(m):
        d, _ = abx_ref.dtw(q, u[s[j]:j + 1], metric)
        assert d.view(np.int32) == e[j].view(np.int32), j
    jb, eb = R.best(e)
    assert eb == e.min() and jb == int(np.argmin(e))


def test_oracle_one_row_query():
    rng = np.random.default_rng(2)
    q, u = rng.standard_normal((1, 6)).astype(np.float32), rng.standard_normal((25, 6)).astype(np.float32)
    for metric in ("angular", "cosine"):
        e, s, gap = R.sdtw(q, u, metric)
        assert np.array_equal(e.view(np.int32), abx_ref.frame_costs(q, u, metric)[0].view(np.int32))
        assert s.tolist() == list(range(25)) and np.all(np.isinf(gap))
