"""Segmentation without a GPU: the float64 oracle of tests/segment_ref.py against brute force over all cuts (cost, and the tie
order on integer scores), its limits in lambda, planted cases; segment.boundary_scores and to_items on hand-made cases;
SEG_SIGNATURES against include/fhvae_segment.h and the built library, fhvae_seg_ws_bytes and the argument errors of the two
calls (they return before any launch); and the command lines with the GPU part stubbed: without --segment / --units-segment
every output is byte for byte what it is with the flag's code absent, with it the new files and the "segments" block appear."""
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import ext_abi
import segment_ref as R
from ext_abi import swap as _swap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, ALIGN, LIMIT = -1, -2, -4, -5


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import segment

    return segment.load_library()


# ------------------------------------------------------------------------------------------------------------------- oracle
def test_oracle_dp_equals_brute_force():
    """T <= 10, K <= 3, Lmax in {1, 2, 3, T}, lambda in {0, 0.3, 10}: the recursion's cost is the minimum over all 2^(T-1) cuts
    (to float64 rounding: the two add in different orders), and the cost of its own segmentation is that minimum."""
    rng = np.random.default_rng(3)
    n = 0
    for T in range(0, 11):
        for K in (1, 2, 3):
            for L in sorted({1, 2, 3, max(T, 1)}):
                for lam in (0.0, 0.3, 10.0):
                    x = rng.standard_normal((T, 16)).astype(np.float32)
                    cent = rng.standard_normal((K, 16)).astype(np.float32)
                    score, unit, _, _ = R.scores(x, cent, L)
                    starts, units, cost, flag = R.dp(score, unit, lam)
                    want, _ = R.brute_force(score, lam, L)
                    tol = 1e-12 * max(1.0, abs(want))
                    assert flag == 0 and abs(cost - want) <= tol, (T, K, L, lam)
                    assert abs(R.objective(x, cent, starts, units, lam) - want) <= 1e-10 * max(1.0, abs(want)), (T, K, L, lam)
                    if T:
                        lens = np.diff(np.concatenate([starts, [T]]))
                        assert starts[0] == 0 and (lens >= 1).all() and (lens <= L).all()
                    n += 1
    assert n == 360  # (T = 0 .. 3 repeat an Lmax)


def test_oracle_tie_order_on_integer_scores():
    """Integer scores and dyadic lambdas: every sum is exact and ties abound.  The recursion's cut is the brute force's first in
    the order "smallest l from the last segment backwards", and the costs agree bit for bit."""
    rng = np.random.default_rng(4)
    ties = 0
    for T in range(1, 11):
        for L in sorted({1, 2, 3, T}):
            for lam in (0.0, 0.25, 4.0):
                score = rng.integers(-2, 3, size=(T, L)).astype(np.float32)
                for n in range(T):
                    score[n, n + 1:] = np.inf
                unit = rng.integers(0, 3, size=(T, L)).astype(np.int32)
                starts, units, cost, flag = R.dp(score, unit, lam)
                want, arg = R.brute_force(score, lam, L)
                assert flag == 0 and cost == want and starts.tolist() == arg, (T, L, lam)
                ends = arg[1:] + [T]
                assert units.tolist() == [int(unit[b - 1, b - a - 1]) for a, b in zip(arg, ends)]
                ties += 1
    assert ties > 90
    # all-zero scores, lambda 0: every cut costs 0; the smallest l wins at every step: one frame per segment
    starts, _, cost, _ = R.dp(np.zeros((5, 3), np.float32), np.zeros((5, 3), np.int32), 0.0)
    assert starts.tolist() == [0, 1, 2, 3, 4] and cost == 0.0
    # +inf and NaN never win; nothing but them: not finite
    score = np.array([[1.0, np.inf], [np.nan, 2.0], [np.inf, np.nan]], dtype=np.float32)
    assert R.dp(score, np.zeros((3, 2), np.int32), 0.5)[3] == R.NOT_FINITE
    score[2, 0] = 3.0
    starts, _, cost, flag = R.dp(score, np.zeros((3, 2), np.int32), 0.5)
    assert flag == 0 and starts.tolist() == [0, 2] and cost == (0.0 + 2.0 + 0.5) + 3.0 + 0.5
    assert R.dp(np.zeros((0, 4), np.float32), np.zeros((0, 4), np.int32), 1.0)[2:] == (0.0, 0)


def test_lambda_limits():
    rng = np.random.default_rng(5)
    for T, K, L in ((1, 1, 1), (7, 3, 3), (10, 2, 4), (23, 5, 7), (64, 3, 64), (65, 3, 64)):
        x = rng.standard_normal((T, 16)).astype(np.float32)
        cent = rng.standard_normal((K, 16)).astype(np.float32)
        score, unit, _, _ = R.scores(x, cent, L)
        # lambda = 0: a segment's score for unit k is the sum of its frames' scores for k, so cutting never costs: J* is the sum of
        # the per-frame minima, to float64 rounding
        _, _, cost, _ = R.dp(score, unit, 0.0)
        frames = float(score[:, 0].sum())
        assert abs(cost - frames) <= 1e-12 * np.abs(score[:, 0]).sum(), (T, K, L)
        # a large lambda: as few segments as Lmax allows
        starts, _, _, _ = R.dp(score, unit, 1e9)
        assert len(starts) == -(-T // L), (T, K, L)


def test_planted_cases_are_recovered():
    rng = np.random.default_rng(6)
    for K, D, L in ((2, 16, 1), (17, 32, 5), (65, 32, 8)):
        x, cent, lengths, truth = R.planted(rng, 6, K, D, L)
        ptr = np.concatenate([[0], np.cumsum(lengths)])
        for u, (want_starts, want_units) in enumerate(truth):
            score, unit, gap, B = R.scores(x[ptr[u]:ptr[u + 1]], cent, L)
            starts, units, _, flag = R.dp(score, unit, 0.1)
            assert flag == 0 and starts.tolist() == want_starts.tolist() and units.tolist() == want_units.tolist(), (K, u)


def test_scores_by_hand():
    x = np.zeros((3, 16), dtype=np.float32)
    x[:, 0] = [1.0, 2.0, 4.0]
    cent = np.zeros((3, 16), dtype=np.float32)
    cent[:, 0] = [0.0, 2.0, 2.0]  # (two equal centroids: the first wins)
    score, unit, gap, B = R.scores_loops(x, cent, 2)
    # l |c|^2 - 2 S c: row 0, l = 1: (0, 4 - 4, .) -> 0 at k = 0; row 1: l = 1: (0, 4 - 8) = -4; l = 2: S = 3: (0, 8 - 12) = -4
    assert score.tolist() == [[0.0, np.inf], [-4.0, -4.0], [-12.0, -16.0]]
    assert unit.tolist() == [[0, -1], [1, 1], [1, 1]]
    assert gap[1].tolist() == [0.0, 0.0] and gap[0, 0] == 0.0 and gap[0, 1] == np.inf
    assert B[2, 1] == 2.0 ** -23 * 18 * (36.0 / 2 + 2 * 4.0) and B[0, 1] == 0.0
    nan = x.copy()
    nan[1, 3] = np.nan
    for f in (R.scores, R.scores_loops):
        score, unit, _, _ = f(nan, cent, 2)
        assert score[1].tolist() == [np.inf, np.inf] and unit[1].tolist() == [0, 0] and score[2, 1] == np.inf and np.isfinite(score[2, 0])
    # the vectorised form the GPU tests use: the loops' values to float64 rounding (its dots are a matrix product's)
    rng = np.random.default_rng(9)
    for T, K, D, L in ((1, 1, 16, 1), (9, 3, 16, 4), (20, 17, 32, 64), (13, 2, 48, 5)):
        xs, cs = rng.standard_normal((T, D)).astype(np.float32), rng.standard_normal((K, D)).astype(np.float32)
        if K > 2:
            cs[2] = cs[0]
        got, want = R.scores(xs, cs, L), R.scores_loops(xs, cs, L)
        fin = np.isfinite(want[0])
        assert np.array_equal(fin, np.isfinite(got[0])) and np.array_equal(got[1][~fin], want[1][~fin])
        assert np.abs(got[0][fin] - want[0][fin]).max() <= 1e-12 * np.abs(want[0][fin]).max()
        clear = fin & (want[2] > 1e-9)
        assert np.array_equal(got[1][clear], want[1][clear]) and (got[1][fin] >= 0).all()
        assert np.allclose(got[2][clear], want[2][clear], rtol=0, atol=1e-11) and np.allclose(got[3], want[3], rtol=1e-12, atol=0)
        if K > 2:
            assert (got[1] != 2).all() and (want[1] != 2).all()  # (a duplicate row: the smaller index)
    assert score[1].tolist() == [np.inf, np.inf] and unit[1].tolist() == [0, 0] and score[2, 1] == np.inf and np.isfinite(score[2, 0])


def test_the_gpu_cases_stay_clear_of_ties():
    """What tests/test_segment_gpu.py asserts of its inputs, checked here with the oracle alone: at most 1 % of a case's finite
    cells have their runner-up within 2 B of the best (observed: at most 0.2 %), and the sweep is the issue's."""
    import segment_cases as SC

    worst = max(SC.inside_gap(SC.case(name)) for name in SC.NAMES)
    print("the largest share of cells within 2 B of a tie: %.4f" % worst)
    assert worst <= 0.01
    assert {(SC.SPECS[n]["L"], SC.SPECS[n]["K"]) for n in SC.NAMES if SC.SPECS[n]["D"] == 32} >= {(L, K) for L in (1, 2, 5, 32, 64) for K in (1, 2, 17, 65)}
    assert {SC.SPECS[n]["D"] for n in SC.NAMES} == {16, 32, 80, 128}
    for L in (1, 2, 5, 32, 64):
        assert set(SC.lengths_for(L)) == {0, 1, 2, max(L - 1, 0), L, L + 1, 63, 64, 65, 300}


# ------------------------------------------------------------------------------------------------------------ host functions
def _item(key, on, off=None, phone="a"):
    return (key, on, on + 0.01 if off is None else off, phone, "-", "-", "s")


def test_boundary_scores_on_hand_made_cases():
    import segment

    # reference: tokens at 0, 0.10, 0.20, 0.30 -> interior onsets 0.10, 0.20, 0.30.  The boundary in front of frame f stands at
    # (f - 0.5) * 0.010: frame 10 -> 0.095
    ref = [_item("u", 0.0), _item("u", 0.105), _item("u", 0.205), _item("u", 0.305)]
    perfect = segment.boundary_scores([np.array([0, 11, 21, 31])], ref, ["u"], [40])
    assert perfect["precision"] == perfect["recall"] == perfect["f"] == 1.0 and perfect["os"] == 0.0
    assert perfect["r_value"] == pytest.approx(1.0) and (perfect["hits"], perfect["hyp_boundaries"], perfect["ref_boundaries"]) == (3, 3, 3)
    assert perfect["utterances"] == 1
    # shifted by exactly tol (two frames): still hits; by tol and one frame: none
    by_tol = segment.boundary_scores([np.array([0, 13, 23, 33])], ref, ["u"], [40])
    assert by_tol["hits"] == 3 and by_tol["precision"] == 1.0
    beyond = segment.boundary_scores([np.array([0, 14, 24, 34])], ref, ["u"], [40])
    assert beyond["hits"] == 0 and beyond["precision"] == 0.0 and beyond["recall"] == 0.0 and beyond["f"] == 0.0
    assert beyond["os"] is None and beyond["r_value"] is None
    early = segment.boundary_scores([np.array([0, 9, 19, 29])], ref, ["u"], [40])
    assert early["hits"] == 3
    assert segment.boundary_scores([np.array([0, 8, 18, 28])], ref, ["u"], [40])["hits"] == 0
    # two hypotheses near one reference: the reference is hit once
    two = segment.boundary_scores([np.array([0, 10, 12])], [_item("u", 0.0), _item("u", 0.105)], ["u"], [40])
    assert (two["hits"], two["hyp_boundaries"], two["ref_boundaries"]) == (1, 2, 1)
    assert two["precision"] == 0.5 and two["recall"] == 1.0 and two["f"] == pytest.approx(2 / 3) and two["os"] == 1.0
    r1, r2 = math.sqrt(0.0 + 1.0), (1.0 - 1.0 - 1.0) / math.sqrt(2.0)
    assert two["r_value"] == pytest.approx(1.0 - (abs(r1) + abs(r2)) / 2.0)
    # half the boundaries found, none invented: os = -0.5
    half = segment.boundary_scores([np.array([0, 11])], ref[:3], ["u"], [40])
    assert half["precision"] == 1.0 and half["recall"] == 0.5 and half["os"] == -0.5
    r1, r2 = math.sqrt(0.25 + 0.25), (0.5 - 1.0 + 0.5) / math.sqrt(2.0)
    assert half["r_value"] == pytest.approx(1.0 - (r1 + abs(r2)) / 2.0)
    # empty sides
    none_h = segment.boundary_scores([np.array([0])], ref, ["u"], [40])
    assert none_h["precision"] is None and none_h["recall"] == 0.0 and none_h["f"] is None and none_h["hyp_boundaries"] == 0
    none_r = segment.boundary_scores([np.array([0, 5])], ref[:1], ["u"], [40])
    assert none_r["recall"] is None and none_r["precision"] == 0.0 and none_r["f"] is None and none_r["ref_boundaries"] == 0
    both = segment.boundary_scores([np.array([0])], ref[:1], ["u"], [40])
    assert both["precision"] is None and both["recall"] is None and both["r_value"] is None
    # an utterance the items do not hold is left out; the items' order within an utterance does not matter; Kaldi's frame offset
    got = segment.boundary_scores([np.array([0, 11, 21, 31]), np.array([0, 3])], ref[::-1], ["u", "v"], [40, 9])
    assert got["utterances"] == 1 and got["hits"] == 3 and got["hyp_boundaries"] == 3
    off = segment.boundary_scores([np.array([0, 10])], [_item("u", 0.0), _item("u", 0.1075)], ["u"], [40], 0.020, 0.010, 0.0125)
    assert off["hits"] == 1
    with pytest.raises(ValueError):
        segment.boundary_scores([np.array([0])], ref, ["u", "v"], [40, 9])
    # the oracle's sweep on the same cases
    assert R.boundary_scores([[0.095, 0.115]], [[0.105]], 0.020) == (1, 2, 1)


def test_to_items_round_trips_through_the_item_file(tmp_path):
    import abx
    import segment

    keys, spk, lengths = ["u1", "u2", "u3"], ["s1", "-", "s2"], [40, 0, 1]
    segs = [(np.array([0, 5, 6, 31]), np.array([7, 0, 7, 12], dtype=np.int32)), (np.zeros(0, np.int64), np.zeros(0, np.int32)),
            (np.array([0]), np.array([3], dtype=np.int32))]
    for shift, offset in ((0.010, 0.0), (0.0125, 0.005), (0.010, 0.0125)):
        its = segment.to_items(keys, spk, segs, lengths, shift, offset)
        assert [it[0] for it in its] == ["u1"] * 4 + ["u3"] and [it[3] for it in its] == ["u7", "u0", "u7", "u12", "u3"]
        assert [(it[4], it[5]) for it in its] == [("-", "u0"), ("u7", "u7"), ("u0", "u12"), ("u7", "-"), ("-", "-")]
        assert [it[6] for it in its] == ["s1"] * 4 + ["s2"]
        path = str(tmp_path / "segments.item")
        abx.write_items(path, its)
        back = abx.read_items(path)
        assert [it[3:] for it in back] == [it[3:] for it in its]
        got = [abx.frame_range(it[1], it[2], 40 if it[0] == "u1" else 1, shift, offset) for it in back]
        assert got == [(0, 5), (5, 1), (6, 25), (31, 9), (0, 1)]
    assert [u.tolist() for u in segment.frame_units(segs, lengths)] == [[7] * 5 + [0] + [7] * 25 + [12] * 9, [], [3]]
    with pytest.raises(ValueError):
        segment.to_items(keys, spk[:2], segs, lengths)


def test_calls_refuse_cpu_tensors_and_bad_arguments():
    import segment

    x, cent, ptr = torch.zeros(4, 16), torch.zeros(2, 16), torch.tensor([0, 4])
    with pytest.raises(RuntimeError, match="device tensor"):
        segment.scores(x, cent, ptr, 4)
    with pytest.raises(RuntimeError, match="device tensor"):
        segment.dp(torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.int32), ptr, 1.0)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="max_len"):
            segment.segment(x, cent, [4], 1.0, bad)
    with pytest.raises(ValueError, match="rows"):
        segment.segment(x, cent, [3], 1.0, 4)


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_signatures_match_the_header():
    import hip_binding as hb
    import segment

    text = ext_abi.header_text("fhvae_segment.h")
    found = ext_abi.declared("fhvae_segment.h", "fhvae_seg_")
    assert found == segment.SEG_SIGNATURES and sorted(found) == ["fhvae_seg_dp", "fhvae_seg_scores", "fhvae_seg_ws_bytes"]
    assert not set(found) & set(hb.SIGNATURES)
    assert int(re.search(r"#define FHVAE_SEG_MAX_LEN (\d+)", text).group(1)) == segment.SEG_MAX_LEN == R.MAX_LEN == 64
    assert int(re.search(r"#define FHVAE_SEG_CHUNK_ROWS (\d+)", text).group(1)) == segment.SEG_CHUNK_ROWS
    for name, value in (("FHVAE_SEG_BAD_PTR", segment.SEG_BAD_PTR), ("FHVAE_SEG_NOT_FINITE", segment.SEG_NOT_FINITE)):
        assert int(re.search(r"%s = (\d+)" % name, text).group(1)) == value
    assert (segment.SEG_BAD_PTR, segment.SEG_NOT_FINITE) == (R.BAD_PTR, R.NOT_FINITE)


def test_symbols_exported_and_the_main_header_untouched(lib):
    import hip_binding as hb
    import segment

    for name in segment.SEG_SIGNATURES:
        assert hasattr(lib, name) and name not in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12 and len(hb.SIGNATURES) == 81  # include/fhvae_hip.h is untouched
    assert "fhvae_seg_" not in open(os.path.join(ROOT, "include", "fhvae_hip.h")).read().lower()


def test_workspace_is_positive_and_monotone(lib):
    f = lib.fhvae_seg_ws_bytes
    sizes = {"N": (1, 2, 255, 256, 4095, 4096, 4097, 360000, 1 << 30), "K": (1, 2, 63, 64, 65, 1000, 1 << 20), "D": (16, 32, 48, 80, 128),
             "L": (1, 2, 5, 16, 32, 63, 64)}
    base = {"N": 5000, "K": 100, "D": 32, "L": 16}
    for name, values in sizes.items():
        last = 0
        for v in values:
            a = dict(base, **{name: v})
            got = f(a["N"], a["K"], a["D"], a["L"])
            assert got > 0 and got >= last and got % 256 == 0, (name, v)
            last = got
    # the segment sums are a chunk's, not the call's: above the chunk the workspace grows by the row bookkeeping alone
    assert f(1 << 30, 100, 32, 64) - f(4096, 100, 32, 64) < 5 * (1 << 30) and f(1 << 30, 100, 128, 64) < (1 << 30) * 4 + (1 << 28)
    assert f(4096, 100, 32, 64) >= 4096 * 64 * 32 * 4
    for bad in ((0, 10, 32, 8), (10, 0, 32, 8), ((1 << 30) + 1, 10, 32, 8), (10, (1 << 20) + 1, 32, 8), (10, 10, 8, 8), (10, 10, 136, 8),
                (10, 10, 40, 8), (10, 10, 32, 0), (10, 10, 32, 65), (10, 10, 32, -1)):
        assert f(*bad) == 0, bad


def test_scores_errors_before_any_launch(lib):
    keep, p = ext_abi.aligned()
    ws = lib.fhvae_seg_ws_bytes(4, 2, 32, 3)
    fn = lib.fhvae_seg_scores
    #       x ldx N  D  cent ldc K Lmax utt_ptr U ws ws_bytes score unit status stream
    good = [p, 32, 4, 32, p, 32, 2, 3, p, 1, p, ws, p, p, p, None]
    for i in (0, 4, 8, 10, 12, 13, 14):
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((3, 8), (3, 136), (3, 40), (3, 0), (1, 28), (5, 16), (2, 0), (2, -1), (6, 0), (6, -3), (9, 0), (9, -1), (11, ws - 1), (11, 0)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i, bad in ((0, p + 4), (4, p + 8), (1, 34), (5, 33), (8, p + 4), (10, p + 8), (12, p + 2), (13, p + 1), (14, p + 2)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    for i, bad in ((2, (1 << 30) + 1), (6, (1 << 20) + 1), (7, 0), (7, 65), (7, -1), (9, 1 << 31)):
        assert fn(*_swap(good, i, bad)) == LIMIT, (i, bad)
    del keep


def test_dp_errors_before_any_launch(lib):
    keep, p = ext_abi.aligned()
    fn = lib.fhvae_seg_dp
    #       score unit N Lmax utt_ptr U lambda ws ws_bytes seg_unit seg_start n_seg cost status stream
    good = [p, p, 10, 3, p, 2, 0.5, p, 256, p, p, p, p, p, None]
    for i in (0, 1, 4, 7, 9, 10, 11, 12, 13):
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((2, -1), (5, 0), (5, -2), (6, -0.5), (6, float("nan")), (8, 9), (8, -1)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i, bad in ((0, p + 2), (1, p + 1), (4, p + 4), (7, p + 8), (9, p + 2), (11, p + 2), (12, p + 4), (13, p + 2)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    for i, bad in ((2, (1 << 30) + 1), (3, 0), (3, 65), (5, 1 << 31)):
        assert fn(*_swap(_swap(good, 8, 1 << 40), i, bad)) == LIMIT, (i, bad)
    del keep


# --------------------------------------------------------------------------------------------------------------------- CLI
KEYS, LENGTHS = ["s1-a", "s1-b", "s2-c"], [7, 0, 5]


def _corpus():
    rng = np.random.default_rng(11)
    cent = np.zeros((3, 16), dtype=np.float32)
    cent[0, 0], cent[1, 1], cent[2, 2] = 2.0, 2.0, 2.0
    frames = [0, 0, 0, 1, 1, 2, 2] + [2, 2, 2, 0, 0]
    rows = cent[frames] + 0.01 * rng.standard_normal((12, 16)).astype(np.float32)
    return rows.astype(np.float32), cent, np.asarray(frames, dtype=np.int32)


def _stub_gpu(monkeypatch):
    """Everything that needs a device, replaced: the rows and the per-frame units are fixed, the segmentation is the oracle's."""
    import frames
    import segment
    import units

    rows, cent, labels = _corpus()
    info = {"on": "z1", "k": 3, "frames": 12, "iterations": 2, "converged": True, "inertia": 0.5, "reseeded": 0, "seed": 0}

    def discover(rows_, width, keys, lengths, on, **kw):
        ptr = np.concatenate([[0], np.cumsum(lengths)])
        seqs = [labels[int(a):int(b)] for a, b in zip(ptr[:-1], ptr[1:])]
        out = dict(info, on=on)
        out.update(units.bitrate(seqs, kw.get("frame_shift", 0.010)))
        return out, cent[:, :width].copy(), np.bincount(labels, minlength=3).astype(np.int64), seqs

    def segment_stub(x, table, lengths, lam, max_len, ws_limit=1 << 30):
        ptr = np.concatenate([[0], np.cumsum(lengths)])
        segs, costs = [], []
        for a, b in zip(ptr[:-1], ptr[1:]):
            score, unit, _, _ = R.scores(x[int(a):int(b)].numpy(), table.numpy(), max_len)
            starts, un, cost, flag = R.dp(score, unit, lam)
            assert flag == 0
            segs.append((starts, un))
            costs.append(cost)
        return segs, np.asarray(costs)

    monkeypatch.setattr(frames, "pool_from_scp", lambda *a, **k: types.SimpleNamespace(keys=KEYS, lengths=LENGTHS))
    monkeypatch.setattr(units, "corpus_rows", lambda model, pool, on, batch: (torch.from_numpy(rows), 16))
    monkeypatch.setattr(units, "discover", discover)
    monkeypatch.setattr(segment, "segment", segment_stub)
    return info


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


UNITS_JSON = """{
 "on": "z1",
 "k": 3,
 "frames": 12,
 "iterations": 2,
 "converged": true,
 "inertia": 0.5,
 "reseeded": 0,
 "seed": 0,
 "bitrate": %s,
 "bitrate_collapsed": %s
}"""


def test_discover_units_outputs_with_and_without_segment(tmp_path, monkeypatch, capsys):
    import discover_units as DU
    import hip_binding as hb
    import units
    import utils

    _stub_gpu(monkeypatch)

    class Model:
        seg_len, model = 20, "fhvae"

        def eval(self):
            return self

        def to(self, dev):
            return self

    monkeypatch.setattr(utils, "load_checkpoint_file", lambda path, finetune=True: (Model(),))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(hb, "lstm_sync_status", lambda: 0)
    item = tmp_path / "ref.item"
    item.write_text("#file onset offset #phone prev-phone next-phone speaker\n"
                    "s1-a 0.000 0.020 p0 - p1 s1\ns1-a 0.030 0.040 p1 p0 p2 s1\ns1-a 0.050 0.060 p2 p1 - s1\n"
                    "s2-c 0.000 0.020 p2 - p0 s2\ns2-c 0.030 0.040 p0 p2 - s2\n")
    base = ["--checkpoint", "c.tar", "--feat-scp", "f.scp", "--len-scp", "l.scp", "--k", "3"]
    plain, seg, seg_item = str(tmp_path / "plain"), str(tmp_path / "seg"), str(tmp_path / "seg_item")
    assert DU.main(base + ["--out", plain]) == 0
    assert DU.main(base + ["--out", seg, "--segment", "--dur-penalty", "0.1", "--max-seg-frames", "4"]) == 0
    assert DU.main(base + ["--out", seg_item, "--segment", "--dur-penalty", "0.1", "--max-seg-frames", "4", "--item", str(item)]) == 0
    capsys.readouterr()
    a, b, c = _files(plain), _files(seg), _files(seg_item)
    # without the flag: the five files of before, with the bytes of before
    assert sorted(a) == ["units.json", "units.txt", "units_centroids.npy", "units_collapsed.txt", "units_counts.npy"]
    rate = units.bitrate([[0, 0, 0, 1, 1, 2, 2], [], [2, 2, 2, 0, 0]], 0.010)
    assert a["units.json"].decode() == UNITS_JSON % (json.dumps(rate["bitrate"]), json.dumps(rate["bitrate_collapsed"]))
    assert a["units.txt"] == b"s1-a 0 0 0 1 1 2 2\ns1-b\ns2-c 2 2 2 0 0\n" and a["units_collapsed.txt"] == b"s1-a 0 1 2\ns1-b\ns2-c 2 0\n"
    # with it: the same five but for the added "segments" entry, and the two new files
    assert sorted(b) == sorted(list(a) + ["segments.item", "segments.txt"])
    for name in a:
        if name != "units.json":
            assert a[name] == b[name] == c[name], name
    info = json.loads(b["units.json"])
    block = info.pop("segments")
    assert json.dumps(info, indent=1) == a["units.json"].decode() and list(json.loads(b["units.json"]))[-1] == "segments"
    assert b["segments.txt"] == b"s1-a 0 1 2\ns1-b\ns2-c 2 0\n"
    assert list(block) == ["dur_penalty", "max_seg_frames", "segments", "mean_frames", "cost", "bitrate_segments"]
    assert (block["dur_penalty"], block["max_seg_frames"], block["segments"], block["mean_frames"]) == (0.1, 4, 5, 12 / 5)
    assert block["bitrate_segments"] == units._bits([[0, 1, 2], [], [2, 0]], 0.12) and block["cost"] < 0
    import abx

    its = abx.read_items(os.path.join(seg, "segments.item"))
    assert [(it[0], it[3], it[4], it[5], it[6]) for it in its] == [("s1-a", "u0", "-", "u1", "-"), ("s1-a", "u1", "u0", "u2", "-"),
                                                                   ("s1-a", "u2", "u1", "-", "-"), ("s2-c", "u2", "-", "u0", "-"),
                                                                   ("s2-c", "u0", "u2", "-", "-")]
    assert [abx.frame_range(it[1], it[2], 7) for it in its] == [(0, 3), (3, 2), (5, 2), (0, 3), (3, 2)]
    # with --item: the boundary figures and the quality of the segments' units
    withitem = json.loads(c["units.json"])["segments"]
    assert withitem["hits"] == 3 and withitem["precision"] == 1.0 and withitem["recall"] == 1.0 and withitem["r_value"] == pytest.approx(1.0)
    assert withitem["cluster_purity"] == 1.0 and withitem["pnmi"] == pytest.approx(1.0) and withitem["labelled_frames"] == 12
    assert c["segments.item"] == b["segments.item"] and c["segments.txt"] == b["segments.txt"]


def test_eval_model_units_outputs_with_and_without_segment(tmp_path, monkeypatch):
    import eval_model as EM

    _stub_gpu(monkeypatch)
    base = ["--checkpoint", "c.tar", "--feat-scp", "f.scp", "--len-scp", "l.scp", "--units", "3", "--units-on", "z1"]
    out = {}
    for name, extra in (("plain", []), ("seg", ["--units-segment", "--units-dur-penalty", "0.1", "--units-max-seg-frames", "4"])):
        d = tmp_path / name
        d.mkdir()
        args = EM.parse_args(base + ["--out", str(d)] + extra)
        out[name] = (EM.discover_units(args, None, 20, str(d), torch.device("cpu")), _files(str(d)))
    (plain_block, plain), (seg_block, seg) = out["plain"], out["seg"]
    assert sorted(plain) == ["units_centroids_z1.npy", "units_z1.txt"] and "segments" not in plain_block["z1"]
    assert sorted(seg) == ["segments_z1.item", "segments_z1.txt", "units_centroids_z1.npy", "units_z1.txt"]
    assert all(plain[f] == seg[f] for f in plain)
    block = seg_block["z1"].pop("segments")
    assert seg_block == plain_block and block["segments"] == 5 and block["max_seg_frames"] == 4
    assert seg["segments_z1.txt"] == b"s1-a 0 1 2\ns1-b\ns2-c 2 0\n"


def test_command_line_argument_errors(tmp_path, capsys):
    import discover_units as DU
    import eval_model as EM

    base = ["--checkpoint", "c.tar", "--feat-scp", "f.scp", "--len-scp", "l.scp", "--out", str(tmp_path / "o"), "--k", "4"]
    for extra in (["--segment", "--max-seg-frames", "0"], ["--segment", "--max-seg-frames", "65"], ["--dur-penalty", "-1"],
                  ["--boundary-tol", "-0.1"]):
        with pytest.raises(SystemExit) as e:
            DU.main(base + extra)
        assert e.value.code == 2, extra
    args = DU.parse_args(base)[1]
    assert (args.segment, args.dur_penalty, args.max_seg_frames, args.boundary_tol) == (False, 1.0, 32, 0.020)
    ebase = ["--checkpoint", "c.tar", "--out", str(tmp_path / "o"), "--feat-scp", "f.scp", "--len-scp", "l.scp"]
    for extra in (["--units-segment"], ["--units", "4", "--units-max-seg-frames", "65"], ["--units", "4", "--units-dur-penalty", "-2"]):
        with pytest.raises(SystemExit) as e:
            EM.parse_args(ebase + extra)
        assert e.value.code == 2, extra
    capsys.readouterr()
    args = EM.parse_args(ebase + ["--units", "4"])
    assert (args.units_segment, args.units_dur_penalty, args.units_max_seg_frames) == (False, 1.0, 32)
