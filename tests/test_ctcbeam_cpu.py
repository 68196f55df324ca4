"""CTC prefix beam search without a GPU: the float64 oracle of tests/ctcbeam_ref.py against brute-force enumeration of all paths,
with and without a table; its tie order; the condition that lets the GPU test leave nothing out (every case of
tests/ctcbeam_cases.py has an oracle margin of at least 100 times the GPU test's score bound); ctcbeam.bigram, table and the
tie rule of tune; CB_SIGNATURES against include/fhvae_ctcbeam.h and the built library, fhvae_cb_ws_bytes and the argument errors
of fhvae_cb_decode (they return before any launch)."""
import os
import re

import numpy as np
import pytest

import ctc_ref
import ctcbeam_cases as K
import ctcbeam_ref as R
import ext_abi
from ext_abi import swap as _swap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, ALIGN, LIMIT = -1, -2, -4, -5


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import ctcbeam

    return ctcbeam.load_library()


# ------------------------------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("with_table", [False, True])
def test_oracle_against_brute_force(with_table):
    """T <= 5, C <= 3, W = 64: the beam holds every prefix (at most 63), so the search is exact: the hypothesis is the labelling
    of largest total probability (plus the table along it) and its score that sum; without a table the score is -ctc_ref.loss
    of the hypothesis."""
    n = 0
    for z, blank, table in K.small(with_table):
        hyp, score, margin, emptied = R.decode(z, blank, 64, table)
        every = R.brute_force(z, blank, table)
        ranked = sorted(every.items(), key=lambda kv: -kv[1])
        assert not emptied
        assert abs(score - ranked[0][1]) <= 1e-12 * max(1.0, abs(score)), (z, blank, score, ranked[:2])
        if len(ranked) == 1 or ranked[0][1] - ranked[1][1] > 1e-9:
            assert tuple(hyp) == ranked[0][0], (z, blank, hyp, ranked[:2])
            n += 1
        if not with_table:
            assert abs(score + ctc_ref.loss(z, hyp, blank, want_grad=False)[0]) <= 1e-12 * max(1.0, abs(score))
    assert n >= 60


def test_empty_utterance_and_rules_of_the_header():
    rng = np.random.default_rng(2)
    tab = rng.standard_normal((4, 4))
    assert R.decode(np.zeros((0, 3), np.float32), 1, 8)[:2] == ([], 0.0)
    assert R.decode(np.zeros((0, 3), np.float32), 1, 8, tab)[:2] == ([], tab[3][3])
    # the blank at probability 0 and every extension forbidden: the beam empties out
    z = np.array([[0.0, -np.inf, 0.0]], np.float32)
    forbid = np.zeros((4, 4))
    forbid[3, :3] = -np.inf
    assert R.decode(z, 1, 4, forbid) == ([], -np.inf, np.inf, True)
    assert R.decode(z, 1, 4)[3] is False
    # a forbidden repeat: the labelling (0, 0) never appears
    rep = np.zeros((4, 4))
    rep[0, 0] = -np.inf
    z = np.array([[3.0, 0.0, -9.0], [0.0, 3.0, -9.0], [3.0, 0.0, -9.0]], np.float32)
    assert R.decode(z, 1, 8)[0] == [0, 0] and R.decode(z, 1, 8, rep)[0] == [0]
    # class pruning: at class_beam 0 only the arg-max class is open, so a label can only be put out at a frame whose arg-max
    # it is: the hypothesis is a subsequence of the arg-max sequence without its blanks
    z = rng.standard_normal((20, 4)).astype(np.float32)
    hyp, at = R.decode(z, 3, 8, None, 0.0)[0], iter(int(v) for v in z.argmax(axis=1) if v != 3)
    assert hyp and all(any(v == w for w in at) for v in hyp)


def test_beam_one_against_the_greedy_path():
    """The issue states "W = 1 without a table never scores below the greedy labelling's own path".  Under the definition that
    does not hold: when the frame's arg-max is the kept prefix's last label, stay keeps lse(tot + lp[blank], pnb + lp[c]) and
    extend keeps pb + lp[c], and both can lie below tot + lp[c] (by at most log 2).  Measured here: 3 of these 600 random utterances
    (16 of 3000 in a longer run) score below the greedy path, the worst by 0.202.  What holds, and is asserted, is
    score >= greedy path - T log 2; the count of utterances below the greedy path is printed."""
    rng = np.random.default_rng(0)
    below, worst = 0, 0.0
    for trial in range(600):
        C, T = int(rng.integers(2, 6)), int(rng.integers(1, 12))
        blank = int(rng.integers(C))
        z = (rng.standard_normal((T, C)) * rng.choice([0.3, 1, 3])).astype(np.float32)
        score = R.decode(z, blank, 1)[1]
        greedy = ctc_ref.log_softmax(z).max(axis=1).sum()
        assert score >= greedy - T * np.log(2.0) - 1e-12
        below += score < greedy - 1e-12
        worst = max(worst, greedy - score)
    print("beam 1 below the greedy path: %d of 600, worst by %.3f" % (below, worst))


def test_tie_order_at_one_frame():
    """T = 1 with duplicated logits: the extensions of the empty prefix score lp[c] + 0, equal bit for bit, so the smaller
    candidate index (the smaller class) is kept.  The end column then tells which labels were in the beam."""
    z = np.array([[0.0, 1.0, 1.0, 1.0, 1.0]], np.float32)
    end = np.zeros((6, 6))
    end[2, 5], end[4, 5] = 1.0, 5.0
    for W, want in ((1, [1]), (2, [2]), (3, [2]), (4, [4]), (64, [4])):
        assert R.decode(z, 0, W, end)[0] == want, W
    assert R.decode(z, 0, 2)[0] == [1]  # equal final scores: the first beam position
    assert R.decode(z, 0, 2)[2] == 0.0  # and the oracle reports the tie as a margin of 0


# ------------------------------------------------------------------------------------------------- the GPU test's condition
@pytest.mark.parametrize("name", K.ALL)
def test_every_case_has_a_margin_of_100_bounds(name):
    """The GPU test compares every utterance's hypothesis exactly.  That is sound where no decision of the search is closer
    than the scores can err: margin >= 100 * 5 T 2^-53 max(1, |score|).  A seed that fails is replaced in ctcbeam_cases.SEEDS."""
    c = K.case(name)
    hyps, scores, margins, status, _ = K.oracle(name)
    assert status == 0
    for u, T in enumerate(c["lengths"]):
        assert len(hyps[u]) <= T
        if T == 0:
            assert hyps[u] == [] and scores[u] == (c["table"][c["C"]][c["C"]] if c["table"] is not None else 0.0)
            continue
        assert np.isfinite(scores[u]) and margins[u] >= 100.0 * K.bound(T, scores[u]), (name, u, T, margins[u], K.bound(T, scores[u]))


def test_the_grid_covers_what_the_issue_lists():
    cases = [K.case(n) for n in K.GRID]
    assert {c["C"] for c in cases} == set(K.CLASSES) and {c["W"] for c in cases} == set(K.BEAMS)
    assert {T for c in cases for T in c["lengths"]} == set(K.LENGTHS)
    for C in K.CLASSES:
        assert {c["blank"] for c in cases if c["C"] == C} == {0, C // 2, C - 1}
    assert {(c["scale"], c["table"] is None, np.isinf(c["class_beam"])) for c in cases} >= {
        (s, t, b) for s in K.SCALES for t in (False, True) for b in (False,)} | {(1.0, True, True), (50.0, False, True)}
    assert all(0 in c["lengths"][1:-1] or len(c["lengths"]) == 3 for c in cases)


def test_the_recreated_prefix_regime_recreates_prefixes():
    """C = 5, W = 64, T = 130: prefixes fall out of the beam while a child stays and come back.  An implementation that
    identifies a prefix by the node it was created as splits its mass there."""
    for name in K.RECREATE:
        assert K.oracle(name)[4]["recreated"] >= 8, name
    hyps = K.oracle("never-fills")[0]
    assert all(len(h) <= 3 for h in hyps)


# ------------------------------------------------------------------------------------------------------------ host functions
def test_bigram():
    import ctcbeam

    lm = ctcbeam.bigram([[0, 1, 1], [1], []], 3, 2, smooth=1.0)
    assert lm.shape == (4, 4) and lm.dtype == np.float64
    assert np.isneginf(lm[2]).all() and np.isneginf(lm[:, 2]).all()
    p = np.exp(lm)
    assert np.allclose(p[[0, 1, 3]].sum(axis=1), 1.0)  # a row is a distribution over the labels and the end
    # start row: 0 once, 1 once, end once (the empty transcription), smooth 1 on each of the three
    assert np.allclose(p[3], [2 / 6, 2 / 6, 0, 2 / 6])
    assert np.allclose(p[1], [1 / 6, 2 / 6, 0, 3 / 6]) and np.allclose(p[0], [1 / 4, 2 / 4, 0, 1 / 4])
    hard = ctcbeam.bigram([[0, 1]], 3, 2, smooth=0.0)
    assert hard[3, 0] == 0.0 and np.isneginf(hard[3, 1]) and hard[1, 3] == 0.0 and not np.isnan(hard).any()
    for bad in ([[2]], [[3]], [[-1]]):
        with pytest.raises(ValueError):
            ctcbeam.bigram(bad, 3, 2)


def test_table_and_the_tie_rule_of_tune():
    import ctcbeam

    lm = ctcbeam.bigram([[0, 1, 1], [1]], 3, 2)
    t = ctcbeam.table(lm, 0.5, 2.0)
    assert np.array_equal(t[:, 3], 0.5 * lm[:, 3]) and np.array_equal(t[:, :2], 0.5 * lm[:, :2] + 2.0)
    assert np.isneginf(t[2]).all() and np.isneginf(t[:, 2]).all() and not np.isnan(t).any()
    zero = ctcbeam.table(lm, 0.0, 1.0)
    assert np.array_equal(zero[:, :3], np.ones((4, 3))) and not zero[:, 3].any()
    with pytest.raises(ValueError):
        ctcbeam.table(lm, -1.0, 0.0)
    grid = [(1.0, 0.0, 0.2), (0.5, 1.0, 0.1), (0.5, 0.0, 0.1), (0.0, 2.0, 0.1), (0.0, 3.0, 0.1), (1.5, 0.0, 0.3)]
    assert ctcbeam.best_of(grid) == (0.0, 2.0)  # the lowest PER; then the smaller scale; then the smaller bonus
    assert ctcbeam.best_of(grid[:3]) == (0.5, 0.0)
    with pytest.raises(ValueError):
        ctcbeam.best_of([])


def test_decode_refuses_cpu_tensors_and_wrong_dtypes():
    import torch

    import ctcbeam

    z, ptr = torch.zeros(4, 3), torch.tensor([0, 4])
    with pytest.raises(RuntimeError, match="device tensor"):
        ctcbeam.decode(z, ptr, 2)
    with pytest.raises(RuntimeError, match="device tensor"):
        ctcbeam.decode(z.double(), ptr, 2)


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_signatures_match_the_header():
    import ctcbeam
    import hip_binding as hb

    text = ext_abi.header_text("fhvae_ctcbeam.h")
    found = ext_abi.declared("fhvae_ctcbeam.h", "fhvae_")
    assert found == ctcbeam.CB_SIGNATURES and sorted(found) == ["fhvae_cb_decode", "fhvae_cb_ws_bytes"]
    assert not set(found) & set(hb.SIGNATURES)
    assert int(re.search(r"#define FHVAE_CB_MAX_CLASSES (\d+)", text).group(1)) == ctcbeam.CB_MAX_CLASSES == 128
    assert int(re.search(r"#define FHVAE_CB_MAX_BEAM (\d+)", text).group(1)) == ctcbeam.CB_MAX_BEAM == 64
    assert int(re.search(r"#define FHVAE_CB_NODE_BYTES (\d+)", text).group(1)) == ctcbeam.CB_NODE_BYTES == 16
    for name, value in (("FHVAE_CB_BAD_PTR", ctcbeam.CB_BAD_PTR), ("FHVAE_CB_EMPTY", ctcbeam.CB_EMPTY)):
        assert int(re.search(r"%s = (\d+)" % name, text).group(1)) == value
    assert ctcbeam.CB_EMPTY == R.EMPTY


def test_symbols_exported_and_the_main_header_untouched(lib):
    import ctcbeam
    import hip_binding as hb

    for name in ctcbeam.CB_SIGNATURES:
        assert hasattr(lib, name) and name not in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12 and len(hb.SIGNATURES) == 81  # include/fhvae_hip.h is untouched
    assert "fhvae_cb_" not in open(os.path.join(ROOT, "include", "fhvae_hip.h")).read().lower()


def test_workspace_bytes(lib):
    f = lib.fhvae_cb_ws_bytes
    assert f(-1, 8) == 0 and f(10, 0) == 0 and f(10, 65) == 0 and f(10, -1) == 0 and f((1 << 52) + 1, 1) == 0
    assert f(0, 1) == 0 and f(0, 64) == 0
    for W in (1, 2, 63, 64):
        last = 0
        for n in (1, 15, 16, 17, 1000, 3600000, 1 << 40, 1 << 52):
            v = f(n, W)
            assert v >= last and v % 256 == 0 and 16 * n * W <= v < 16 * n * W + 256
            assert W == 1 or v >= f(n, W - 1)  # monotone in the beam too
            last = v


def test_decode_errors_before_any_launch(lib):
    buf, p = ext_abi.aligned()  # (kept alive; the calls below return before anything would read it)
    fn = lib.fhvae_cb_decode
    #       logits ldz n_frames C blank utt_ptr U W class_beam lm hyp hyp_len score status ws ws_bytes stream
    good = [p, 8, 10, 5, 4, p, 2, 8, 1.5, p, p, p, p, p, p, 4096, None]
    assert lib.fhvae_cb_ws_bytes(10, 8) <= 4096
    for i in (0, 5, 10, 11, 12, 13, 14):
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((3, 1), (3, 0), (4, -1), (4, 5), (1, 4), (2, -1), (6, -1), (15, -1), (8, -0.5), (8, float("nan")), (8, float("-inf")),
                   (15, 1024)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i, bad in ((1, 6), (1, 10), (0, p + 4), (0, p + 8), (5, p + 4), (9, p + 4), (10, p + 2), (11, p + 2), (12, p + 4), (13, p + 2),
                   (14, p + 8)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    assert fn(*_swap(_swap(good, 3, 129), 1, 132)) == LIMIT and fn(*_swap(good, 6, 1 << 31)) == LIMIT
    assert fn(*_swap(good, 2, (1 << 52) + 1)) == LIMIT
    for W in (0, -1, 65, 1 << 40):
        assert fn(*_swap(good, 7, W)) == LIMIT, W
    # lm may be NULL, class_beam +inf and 0 are legal: the next refusal is the alignment of score
    assert fn(*_swap(_swap(good, 9, None), 12, p + 4)) == ALIGN
    assert fn(*_swap(_swap(good, 8, float("inf")), 12, p + 4)) == ALIGN and fn(*_swap(_swap(good, 8, 0.0), 12, p + 4)) == ALIGN
    # U == 0: nothing to do, whatever the data pointers are
    assert fn(None, 8, 0, 5, 4, None, 0, 8, 0.0, None, None, None, None, p, None, 0, None) == 0
