"""Forced alignment without a GPU: the float64 oracle of tests/falign_ref.py against brute-force enumeration of all alignments
(score and tie order) and its invariants on random cases; the quality of the definition on the generator's corpus; falign.spans,
items, read_text and boundary_report; FA_SIGNATURES against include/fhvae_falign.h and the built library, fhvae_fa_ws_bytes and
the argument errors of fhvae_fa_align (they return before any launch)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import ctc_ref
import ext_abi
import falign_ref as R
import viterbi_ref as VR
from ext_abi import swap as _swap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, ALIGN, LIMIT = -1, -2, -4, -5


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import falign

    return falign.load_library()


# ------------------------------------------------------------------------------------------------------------------- oracle
def small_cases(integer):
    rng = np.random.default_rng(17 + integer)
    for T in range(1, 7):
        for C in (2, 3):
            for blank in (-1,) + tuple(range(C)):
                classes = [c for c in range(C) if c != blank]
                for L in range(0, 4):
                    if (2 * L + 1 if blank >= 0 else L) ** T > 60000:
                        continue
                    lab = [int(v) for v in rng.choice(classes, size=L)]
                    z = rng.integers(-2, 3, size=(T, C)).astype(np.float32) if integer else rng.standard_normal((T, C)).astype(np.float32)
                    yield z, lab, blank


@pytest.mark.parametrize("integer", [0, 1])
def test_oracle_against_brute_force(integer):
    """T <= 6, L <= 3, C <= 3, both topologies.  On integer logits every sum is exact and ties abound: the oracle's score is the
    maximum and its path the first one in the tie order."""
    n = feasible = 0
    for z, lab, blank in small_cases(integer):
        state, seg, score, flag = R.align(z, lab, blank)
        want, path = R.brute_force(z, lab, blank)
        n += 1
        if path is None:
            assert flag == R.INFEASIBLE and score == -np.inf and (state == -1).all() and (seg == -1).all(), (lab, blank)
            continue
        feasible += 1
        assert flag == 0 and score == want, (z, lab, blank)
        assert state.tolist() == list(path), (z, lab, blank, state, path)
    assert n > 150 and feasible > 60, (n, feasible)


def test_rules_of_the_header():
    rng = np.random.default_rng(5)
    z = rng.standard_normal((6, 4)).astype(np.float32)
    # L = 0 in CTC topology: every state 0, the ordered sum of the blank's scores; HMM topology: infeasible
    state, seg, score, flag = R.align(z, [], 3)
    want = np.float64(z[0, 3])
    for t in range(1, 6):
        want = want + np.float64(z[t, 3])
    assert flag == 0 and score == want and not state.any() and seg.shape == (0, 2)
    assert R.align(z, [], -1)[2:] == (-np.inf, R.INFEASIBLE)
    assert R.align(z[:0], [], 3)[2:] == (0.0, 0) and R.align(z[:0], [], -1)[2:] == (0.0, 0)
    assert R.align(z[:0], [1], 3)[2:] == (-np.inf, R.INFEASIBLE)
    # all-equal labels at T = 2 L - 1: one path; a frame short: none
    state, seg, score, flag = R.align(z[:5], [1, 1, 1], 0)
    assert flag == 0 and state.tolist() == [1, 2, 3, 4, 5] and seg.tolist() == [[0, 0], [2, 2], [4, 4]]
    assert R.align(z[:4], [1, 1, 1], 0)[3] == R.INFEASIBLE
    # HMM at T = L and T = L - 1
    state, seg, score, flag = R.align(z[:3], [1, 1, 2], -1)
    assert flag == 0 and state.tolist() == [0, 1, 2] and seg.tolist() == [[0, 0], [1, 1], [2, 2]]
    assert R.align(z[:2], [1, 1, 2], -1)[3] == R.INFEASIBLE
    # a needed class at -inf, and one that is not needed
    dead = z.copy()
    dead[:, 1] = -np.inf
    assert R.align(dead, [0, 1], 3)[3] == R.INFEASIBLE and R.align(dead, [0, 2], 3)[3] == 0
    # labels the kernel refuses; in HMM topology no class is the blank
    for labels in ([4], [-1], [3], [0] * 257):
        state, seg, score, flag = R.align(rng.standard_normal((600, 4)).astype(np.float32), labels, 3)
        assert flag == R.BAD_LABEL and score == -np.inf and (state == -1).all() and (seg == -1).all()
    assert R.align(z, [3], -1)[3] == 0
    # all-zero scores: every decision is a tie.  The end goes to S - 1, and walking back "stay" wins wherever the state was
    # reachable a frame earlier: the path moves as early as it can
    state, seg, score, flag = R.align(np.zeros((5, 3), np.float32), [1], 0)
    assert state.tolist() == [1, 2, 2, 2, 2] and seg.tolist() == [[0, 0]] and score == 0.0


def test_oracle_invariants_on_random_cases():
    rng = np.random.default_rng(8)
    for trial in range(40):
        C = int(rng.integers(2, 9))
        hmm = trial % 3 == 0
        blank = -1 if hmm else int(rng.integers(C))
        L = int(rng.integers(1, 12))
        classes = [c for c in range(C) if c != blank]
        lab = [int(v) for v in rng.choice(classes, size=L)]
        T = int(rng.integers(2 * L + 1, 2 * L + 30))
        z = rng.standard_normal((T, C)).astype(np.float32)
        state, seg, score, flag = R.align(z, lab, blank)
        assert flag == 0 and R.collapse(state, lab, blank) == lab
        assert (np.diff(state) >= 0).all() and (np.diff(state) <= (1 if hmm else 2)).all()
        ext = R.extended(lab, blank)[0]
        total = np.float64(z[0, ext[state[0]]])
        for t in range(1, T):
            total = total + np.float64(z[t, ext[state[t]]])
        assert total == score  # the path's own sum, added in increasing t
        for i in range(L):
            at = np.nonzero(state == (i if hmm else 2 * i + 1))[0]
            assert at.size and seg[i].tolist() == [at[0], at[-1]] and at[-1] - at[0] + 1 == at.size
        if not hmm:  # the best path's probability is at most the sum over all paths
            nll = ctc_ref.loss(z, lab, blank, want_grad=False)[0]
            lse = ctc_ref.lse(*z.astype(np.float64).T).sum()
            assert score <= -nll + lse + 1e-9 * max(1.0, abs(lse))


# ------------------------------------------------------------------------------------------------------------ host functions
def test_spans_under_both_rules():
    import falign

    # two utterances in CTC topology: blank a a blank b blank blank | nothing aligned; then L = 0
    seg = np.array([[1, 2], [4, 4], [-1, -1]], dtype=np.int32)
    lab_ptr, lengths = [0, 2, 3, 3], [7, 5, 4]
    own = falign.spans(seg, lab_ptr, lengths, "own")
    assert own.tolist() == [[1, 2], [4, 4], [-1, -1]] and own.dtype == np.int64
    assert falign.spans(seg, lab_ptr, lengths, "follow").tolist() == [[1, 3], [4, 6], [-1, -1]]
    assert falign.spans(torch.from_numpy(seg), torch.tensor(lab_ptr), lengths).tolist() == [[1, 3], [4, 6], [-1, -1]]
    # HMM topology: the states tile the frames, the rules agree
    hmm = np.array([[0, 0], [1, 3], [4, 4]], dtype=np.int32)
    assert falign.spans(hmm, [0, 3], [5], "own").tolist() == falign.spans(hmm, [0, 3], [5], "follow").tolist() == hmm.tolist()
    assert falign.spans(np.zeros((0, 2), np.int32), [0, 0], [9]).shape == (0, 2)
    with pytest.raises(ValueError):
        falign.spans(seg, lab_ptr, lengths, "next")
    with pytest.raises(ValueError):
        falign.spans(seg, [0, 2], [7])


def test_items_round_trip_through_the_item_file(tmp_path):
    import abx
    import falign

    names = ["aa", "b", "sil"]
    refs, keys, spk, lengths = [[2, 0, 1, 2], [], [1], [0, 0]], ["u1", "u2", "u3", "u4"], ["s1", "s1", "s2", "s2"], [40, 3, 1, 250]
    sp = np.array([[0, 4], [5, 5], [6, 30], [31, 39], [0, 0], [-1, -1], [-1, -1]])
    for shift, offset in ((0.010, 0.0), (0.0125, 0.005), (0.010, 0.0125)):
        its = falign.items(keys, spk, sp, refs, names, shift, offset)
        assert [it[0] for it in its] == ["u1"] * 4 + ["u3"] and [it[3] for it in its] == ["sil", "aa", "b", "sil", "b"]
        assert [(it[4], it[5]) for it in its] == [("-", "aa"), ("sil", "b"), ("aa", "sil"), ("b", "-"), ("-", "-")]
        assert [it[6] for it in its] == ["s1"] * 4 + ["s2"]
        path = str(tmp_path / "a.item")
        abx.write_items(path, its)
        back = abx.read_items(path)
        got = [abx.frame_range(it[1], it[2], 40 if it[0] == "u1" else 1, shift, offset) for it in back]
        assert got == [(0, 5), (5, 1), (6, 25), (31, 9), (0, 1)]
    with pytest.raises(ValueError):
        falign.items(keys, spk, sp[:-1], refs, names)


def test_read_text(tmp_path):
    import falign

    p = tmp_path / "text"
    p.write_text("u1 a b  c\n\nu2\nu3 a\n")
    assert falign.read_text(str(p)) == (["u1", "u2", "u3"], [["a", "b", "c"], [], ["a"]])
    p.write_text("u1 a\nu2 b\nu1 c\n")
    with pytest.raises(ValueError, match="line 3"):
        falign.read_text(str(p))
    with pytest.raises(OSError):
        falign.read_text(str(tmp_path / "none"))


def test_boundary_report_on_hand_made_items():
    import falign

    ref = [("u1", 0.00, 0.09, "a", "-", "b", "s"), ("u1", 0.10, 0.19, "b", "a", "-", "s"),
           ("u2", 0.00, 0.04, "a", "-", "-", "s"), ("u3", 0.00, 0.04, "a", "-", "-", "s")]
    hyp = [("u1", 0.00, 0.10, "a", "-", "b", "s"), ("u1", 0.11, 0.19, "b", "a", "-", "s"),
           ("u2", 0.03, 0.04, "b", "-", "-", "s"), ("u4", 0.00, 0.04, "a", "-", "-", "s")]
    rep = falign.boundary_report(hyp, ref, 0.010)
    assert rep["utterances"] == 1 and rep["tokens"] == 2 and rep["skipped_sequence"] == 1
    assert rep["onset_mae"] == pytest.approx(0.005) and rep["within_10ms"] == 1.0 and rep["within_20ms"] == 1.0
    assert rep["frame_agreement"] == pytest.approx(19 / 20)
    far = [("u1", 0.03, 0.10, "a", "-", "b", "s"), ("u1", 0.11, 0.19, "b", "a", "-", "s")]
    rep = falign.boundary_report(far, ref, 0.010)
    assert rep["within_10ms"] == 0.5 and rep["within_20ms"] == 0.5 and rep["onset_mae"] == pytest.approx(0.02)
    none = falign.boundary_report(hyp[2:], ref, 0.010)
    assert none["tokens"] == 0 and none["onset_mae"] is None and none["frame_agreement"] is None and none["skipped_sequence"] == 1


def test_align_refuses_cpu_tensors_and_wrong_dtypes():
    import falign

    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="device tensor"):
        falign.align(z, torch.tensor([0, 4]), torch.zeros(1, dtype=torch.int32), torch.tensor([0, 1]), 2)
    with pytest.raises(RuntimeError, match="device tensor"):
        falign.scores_of(z, torch.tensor([0, 4]), {"weights": np.eye(3), "bias": np.zeros(3), "mean": np.zeros(3), "std": np.ones(3),
                                                    "classes": np.arange(3.0)})


# ------------------------------------------------------------------------------------------------------------------ quality
@functools.lru_cache(maxsize=None)
def quality():
    """The definition on the generator's corpus, with the true model's log-posteriors as scores: HMM topology, and CTC topology
    with a constant blank column of -3 under the follow rule -> (frame agreement HMM, share of inner boundaries within a frame,
    worst boundary, frame agreement CTC follow over the frames under a token, the frames under none, the rows' arg-max)."""
    import falign

    c = VR.corpus(60, 5, 8, 1.3, 0)
    lp = VR.log_posteriors(c["x"], c["means"], c["sigma"])
    ptr = np.concatenate([[0], np.cumsum(c["lengths"])])
    lab_ptr = np.concatenate([[0], np.cumsum([len(r) for r in c["refs"]])])
    labels = np.concatenate([np.asarray(r, dtype=np.int32) for r in c["refs"]])
    state, seg, score, status = R.batch(lp, ptr, labels, lab_ptr, -1)
    assert status == 0
    frames_ok = near = inner = worst = 0
    for u, ref in enumerate(c["refs"]):
        a, b = int(ptr[u]), int(ptr[u + 1])
        y = c["y"][a:b]
        frames_ok += int((np.asarray(ref)[state[a:b]] == y).sum())
        truth = np.nonzero(np.diff(y))[0] + 1
        got = seg[2 * int(lab_ptr[u]):2 * int(lab_ptr[u + 1])].reshape(-1, 2)[1:, 0]
        assert truth.shape == got.shape
        d = np.abs(truth - got)
        near, inner, worst = near + int((d <= 1).sum()), inner + d.size, max(worst, int(d.max()))
    wide = np.concatenate([lp, np.full((lp.shape[0], 1), -3.0, np.float32)], axis=1)
    cstate, cseg, _, cstatus = R.batch(wide, ptr, labels, lab_ptr, 5)
    assert cstatus == 0
    sp = falign.spans(cseg.reshape(-1, 2), lab_ptr, c["lengths"], "follow")
    ctc_ok = owned = 0
    for u, ref in enumerate(c["refs"]):
        a, b = int(ptr[u]), int(ptr[u + 1])
        got = np.full(b - a, -1)
        for i, tok in enumerate(ref):
            f, l = sp[int(lab_ptr[u]) + i]
            got[f:l + 1] = tok
        ctc_ok += int((got == c["y"][a:b]).sum())
        owned += int((got >= 0).sum())  # (leading blanks belong to no token: those frames have no label to compare)
    N = int(ptr[-1])
    return frames_ok / N, near / inner, worst, ctc_ok / owned, N - owned, float((lp.argmax(axis=1) == c["y"]).mean())


def test_quality_of_the_definition():
    """Observed with the oracle: 0.9789 of the 2419 frames in HMM topology (the rows' arg-max: 0.8152), 0.972 of the inner
    boundaries within one frame (worst: 3 frames).  In CTC topology under the follow rule 2 leading blank frames belong to no
    token; of the 2417 frames under a token the same 0.9789 carry the right label."""
    hmm, near, worst, ctc_follow, unowned, argmax = quality()
    print("frame agreement: HMM %.4f, CTC follow %.4f (%d frames under no token), arg-max %.4f; inner boundaries within a frame %.4f, worst %d"
          % (hmm, ctc_follow, unowned, argmax, near, worst))
    assert hmm >= 0.97 and near >= 0.96
    assert round(ctc_follow, 4) == round(hmm, 4) == 0.9789 and round(argmax, 4) == 0.8152 and worst == 3 and unowned == 2


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_signatures_match_the_header():
    import falign
    import hip_binding as hb

    text = ext_abi.header_text("fhvae_falign.h")
    found = ext_abi.declared("fhvae_falign.h", "fhvae_")
    assert found == falign.FA_SIGNATURES and sorted(found) == ["fhvae_fa_align", "fhvae_fa_ws_bytes"]
    assert not set(found) & set(hb.SIGNATURES)
    assert int(re.search(r"#define FHVAE_FA_MAX_CLASSES (\d+)", text).group(1)) == falign.FA_MAX_CLASSES == 128
    assert int(re.search(r"#define FHVAE_FA_MAX_LABELS (\d+)", text).group(1)) == falign.FA_MAX_LABELS == 256
    for name, value in (("FHVAE_FA_BAD_PTR", falign.FA_BAD_PTR), ("FHVAE_FA_BAD_LABEL", falign.FA_BAD_LABEL), ("FHVAE_FA_INFEASIBLE", falign.FA_INFEASIBLE)):
        assert int(re.search(r"%s = (\d+)" % name, text).group(1)) == value
    assert (falign.FA_BAD_LABEL, falign.FA_INFEASIBLE, falign.FA_MAX_LABELS) == (R.BAD_LABEL, R.INFEASIBLE, R.MAX_LABELS)


def test_symbols_exported_and_the_main_header_untouched(lib):
    import falign
    import hip_binding as hb

    for name in falign.FA_SIGNATURES:
        assert hasattr(lib, name) and name not in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12 and len(hb.SIGNATURES) == 81  # include/fhvae_hip.h is untouched
    assert "fhvae_fa_" not in open(os.path.join(ROOT, "include", "fhvae_hip.h")).read().lower()


def test_workspace_bytes(lib):
    f = lib.fhvae_fa_ws_bytes
    assert f(-1) == 0 and f(0) == 0 and f((1 << 59) + 1) == 0
    last = 0
    for cells in (1, 255, 256, 257, 1000, 360000 * 201, 1 << 40, 1 << 59):
        v = f(cells)
        assert v >= last and v % 256 == 0 and cells <= v < cells + 256  # at most one byte per cell
        last = v


def test_align_errors_before_any_launch(lib):
    buf, p = ext_abi.aligned()  # (kept alive; the calls below return before anything would read it)
    fn = lib.fhvae_fa_align
    #       scores lds n_frames C blank utt_ptr labels lab_ptr cell_ptr U state seg score status ws ws_bytes stream
    good = [p, 8, 10, 5, 4, p, p, p, p, 2, p, p, p, p, p, 4096, None]
    for i in (0, 5, 6, 7, 8, 10, 11, 12, 13, 14):
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((3, 1), (3, 0), (4, -2), (4, 5), (1, 4), (2, -1), (9, -1), (15, -1)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i, bad in ((1, 6), (1, 10), (0, p + 4), (0, p + 8), (5, p + 4), (6, p + 2), (7, p + 4), (8, p + 4), (10, p + 2), (11, p + 2),
                   (12, p + 4), (13, p + 2), (14, p + 8)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    assert fn(*_swap(_swap(good, 3, 129), 1, 132)) == LIMIT and fn(*_swap(good, 9, 1 << 31)) == LIMIT
    assert fn(*_swap(good, 2, (1 << 52) + 1)) == LIMIT
    # blank == -1 is the HMM topology, not an error: the next refusal is the alignment of score
    assert fn(*_swap(_swap(good, 4, -1), 12, p + 4)) == ALIGN
    # U == 0: nothing to do, whatever the data pointers are
    assert fn(None, 8, 0, 5, 4, None, None, None, None, 0, None, None, None, p, None, 0, None) == 0
    del buf
