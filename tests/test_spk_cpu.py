"""The speaker back end without a GPU: spk_backend.fit against the independent float64 oracle of tests/spk_ref.py (the
whitening identities, the closed-form LLR against dense Gaussians, EM's monotone likelihood, PLDA against the raw cosine on
held-out speakers), eer_from_hist's threshold mapping and min_dcf by hand, the condition on the committed cases,
SPK_SIGNATURES against include/fhvae_spk.h and the built library, the argument errors of the five calls (they return before
any launch), the two command lines with the GPU part stubbed, and the parsing errors."""
import json
import os
import re

import numpy as np
import pytest
import torch

import ext_abi
import spk_cases as SC
import spk_ref as R
from ext_abi import swap as _swap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, ALIGN, LIMIT = -1, -2, -4, -5


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import spk_backend

    return spk_backend.load_library()


@pytest.fixture(scope="module")
def planted():
    """40 speakers of about 20 rows, K = 24, one strong nuisance direction in W; 30 held-out speakers of the same model."""
    x, label = R.planted(5, 40, 20, 24)
    xe, le = R.planted(6, 30, 20, 24)
    for t in (x, label, xe, le):
        t.setflags(write=False)
    return x, label, xe, le


def _rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("lda_dim,ln", [(None, False), (None, True), (16, True), (24, False)])
def test_fit_whitens_and_diagonalises(planted, lda_dim, ln):
    import spk_backend as SB

    x, label, _, _ = planted
    be = SB.fit(x, label, lda_dim, ln, plda_iters=10)
    ref = R.fit(x, label, lda_dim, ln, iters=10)
    K1 = 24 if lda_dim is None else lda_dim
    if lda_dim is not None:
        # A_lda (Sw / N) A_lda^T = I with the oracle's own (ridged) scatter
        assert be.A_lda.shape == (lda_dim, 24)
        assert _rel(be.A_lda @ ref["Sw_lda"] @ be.A_lda.T, np.eye(lda_dim)) <= 1e-9
    else:
        assert be.A_lda is None
    # the oracle's W and B (its own EM, explicit inverses, a loop over the classes) under this fit's A_p
    assert be.A_p.shape == (K1, K1) and be.psi.shape == (K1,) and (be.psi >= 0).all() and (np.diff(be.psi) <= 0).all()
    assert _rel(be.A_p @ ref["W"] @ be.A_p.T, np.eye(K1)) <= 1e-9
    assert np.abs(be.A_p @ ref["B"] @ be.A_p.T - np.diag(be.psi)).max() <= 1e-9 * max(1.0, be.psi.max())
    assert _rel(be.m, ref["m"]) <= 1e-12 and _rel(be.m2, ref["m2"]) <= 1e-9 and _rel(be.psi, ref["psi"]) <= 1e-9


def test_closed_form_llr_equals_the_dense_gaussian_ratio(planted):
    import spk_backend as SB

    x, label, xe, _ = planted
    be = SB.fit(x, label, None, True, plda_iters=10)
    ref = R.fit(x, label, None, True, iters=10)
    y, _ = R.transform64(ref, xe[:12])
    u = (y - be.m2) @ be.A_p.T
    p, q, c = SB.plda_terms(be.psi)
    a = -(q * u * u).sum(axis=1)
    closed = (u * p) @ u.T + a[:, None] + a[None, :] + c
    worst = 0.0
    for i in range(12):
        for j in range(12):
            dense = R.llr_dense(y[i], y[j], ref["m2"], ref["B"], ref["W"])
            worst = max(worst, abs(closed[i, j] - dense) / max(1.0, abs(dense)))
    print("closed form against dense Gaussians: %.2e relative" % worst)
    assert worst <= 1e-9
    assert np.abs(closed - closed.T).max() <= 1e-12 * np.abs(closed).max() and (p >= 0).all()


def test_em_does_not_decrease_the_marginal_likelihood():
    """Small classes, K = 4: the summed dense marginal log-likelihood N(0, I (x) W + 1 1^T (x) B) over the iterations of
    spk_backend.plda_em_step (m2 fixed at the global mean)."""
    import spk_backend as SB

    x, label = R.planted(8, 25, 4, 4, nuisance=2.0)
    xs, idx, counts = SB._labelled(x, label, "test")
    m2, mc, Sw, Sb = SB.scatter(xs, idx, counts)
    assert counts.min() >= 1 and (counts == 1).any() or counts.min() > 1  # (speakers with one row take part)
    W, B = Sw / len(xs), Sb / len(counts)

    def loglik(B, W):
        return sum(R.class_loglik(xs[idx == c], m2, B, W) for c in range(len(counts)))

    last = loglik(B, W)
    first = last
    for it in range(12):
        B, W = SB.plda_em_step(B, W, Sw, mc - m2, counts)
        now = loglik(B, W)
        assert now >= last - 1e-9 * abs(last), (it, last, now)
        last = now
    assert last > first
    # the oracle's step (explicit inverses) is the same map
    Bo, Wo = R.em_step(B, W, Sw, mc - m2, counts)
    Bs, Ws = SB.plda_em_step(B, W, Sw, mc - m2, counts)
    assert _rel(Bs, Bo) <= 1e-10 and _rel(Ws, Wo) <= 1e-10


def test_plda_beats_the_raw_cosine_on_held_out_speakers(planted):
    """The oracle's float64 PLDA EER on held-out speakers is below its raw-cosine EER for the committed seed (the nuisance
    direction and the offset of the data sink the cosine); the LDA + cosine column lies between."""
    x, label, xe, le = planted
    i, j, same = R.trials(le)
    cos = R.cosine_scores(xe, i, j)
    eer_cos = R.exact_eer(cos[same], cos[~same])
    ref = R.fit(x, label, None, False, iters=10)
    _, u = R.transform64(ref, xe)
    s = R.llr_closed(ref, u)[i, j]
    eer_plda = R.exact_eer(s[same], s[~same])
    lda = R.fit(x, label, 16, True, iters=10)
    y, _ = R.transform64(lda, xe)
    cl = R.cosine_scores(y, i, j)
    eer_lda = R.exact_eer(cl[same], cl[~same])
    print("EER: raw cosine %.4f, LDA + cosine %.4f, PLDA %.4f" % (eer_cos, eer_lda, eer_plda))
    assert eer_plda < 0.5 * eer_cos and eer_lda < 0.5 * eer_cos


def test_fit_argument_errors_and_file_round_trip(planted, tmp_path):
    import spk_backend as SB

    x, label, xe, _ = planted
    with pytest.raises(ValueError, match="at least 2"):
        SB.fit(x, np.where(label == 3, 3, -1))
    one_each = np.full(len(label), -1)
    one_each[:5] = np.arange(5)
    with pytest.raises(ValueError, match="2 or more"):
        SB.fit(x, one_each)
    for bad in (0, 25, 40):
        with pytest.raises(ValueError, match="lda_dim"):
            SB.fit(x, label, lda_dim=bad)
    with pytest.raises(ValueError, match="finite"):
        SB.fit(np.where(np.arange(len(x))[:, None] == 0, np.nan, x), label)
    # rows with label -1 are ignored
    half = np.where(np.arange(len(label)) % 2 == 0, label, -1)
    a, b = SB.fit(x, half, 8), SB.fit(x[::2], label[::2], 8)
    assert np.array_equal(a.psi, b.psi) and np.array_equal(a.A_lda, b.A_lda)
    path = str(tmp_path / "backend.npz")
    for be in (a, SB.fit(x, label, None, False)):
        be.save(path)
        back = SB.Backend.load(path)
        assert back.length_norm == be.length_norm and (back.A_lda is None) == (be.A_lda is None)
        for name in ("m", "m2", "A_p", "psi", "p", "q"):
            assert np.array_equal(getattr(back, name), getattr(be, name)), name
        assert back.c == be.c and back.tables_f32()["A1"].dtype == np.float32
    np.savez(path, m=a.m)
    with pytest.raises(ValueError, match="missing"):
        SB.Backend.load(path)


# -------------------------------------------------------------------------------------------------------------- the figures
def test_eer_from_hist_threshold_mapping_and_min_dcf():
    import spk_backend as SB
    import verification as V

    # 4 bins over [10, 18): targets high, non-targets low, the classes cross inside bin 1
    hist = np.array([[0, 2, 2, 4], [6, 2, 0, 0]])
    plain = V.eer_from_hist(hist)
    r = SB.eer_from_hist(hist, 10.0, 18.0)
    assert r["eer"] == plain["eer"] and r["crossing_mass"] == plain["crossing_mass"] and (r["lo"], r["hi"]) == (10.0, 18.0)
    assert r["threshold"] == pytest.approx(10.0 + (plain["threshold"] + 1.0) / 2.0 * 8.0)
    # FRR(k) = (0, 0, .25, .5, 1), FAR(k) = (1, .25, 0, 0, 0): they cross between edges 1 and 2 at t = 0.5: EER 0.125 at 10 + 1.5 * 2
    assert r["eer"] == pytest.approx(0.125) and r["threshold"] == pytest.approx(13.0)
    # min over the edges of 0.01 FRR + 0.99 FAR, over min(0.01, 0.99): edge 2 gives 0.0025 / 0.01
    assert r["min_dcf"] == pytest.approx(0.25)
    assert SB.eer_from_hist(hist, 10.0, 18.0, dcf=(0.5, 1.0, 1.0))["min_dcf"] == pytest.approx(0.25)  # edge 1 or 2: 0.125 / 0.5
    assert SB.eer_from_hist(hist, 10.0, 18.0, dcf=(0.5, 1.0, 10.0))["min_dcf"] == pytest.approx(0.125 / 0.5)  # edge 2: no false accept
    # separable classes: no cost at the edge between them
    assert SB.eer_from_hist(np.array([[0, 0, 3, 3], [5, 5, 0, 0]]), -4.0, 4.0)["min_dcf"] == 0.0
    # the identity mapping on [-1, 1)
    assert SB.eer_from_hist(hist, -1.0, 1.0)["threshold"] == pytest.approx(plain["threshold"])
    with pytest.raises(ValueError, match="dcf"):
        SB.eer_from_hist(hist, 0.0, 1.0, dcf=(1.0, 1.0, 1.0))
    # uint64 counts beyond 2^53 stay exact
    big = np.array([[0, 2 ** 60], [2 ** 60, 0]], dtype=np.uint64)
    assert SB.eer_from_hist(big, 0.0, 1.0)["min_dcf"] == 0.0


def test_exact_eer_by_sorting():
    import spk_backend as SB

    rs = np.random.RandomState(2)
    tar, non = rs.randn(400) + 1.5, rs.randn(3000)
    s, t = np.concatenate([tar, non]), np.concatenate([np.ones(400, bool), np.zeros(3000, bool)])
    perm = rs.permutation(len(s))
    r = SB.exact_eer(s[perm], t[perm])
    # the oracle takes the mean of FRR and FAR where they are closest, this one interpolates: one trial of either class apart
    assert abs(r["eer"] - R.exact_eer(tar, non)) <= 1.0 / 400 + 1.0 / 3000
    assert (r["n_target"], r["n_nontarget"]) == (400, 3000)
    frr, far = np.mean(tar < r["threshold"]), np.mean(non >= r["threshold"])
    assert abs(frr - r["eer"]) <= 1.0 / 400 and abs(far - r["eer"]) <= 1.0 / 400
    assert SB.exact_eer([2.0, 3.0, 0.0, 1.0], [True, True, False, False])["eer"] == 0.0
    assert SB.exact_eer([0.0, 1.0, 2.0, 3.0], [True, True, False, False])["eer"] == 1.0
    with pytest.raises(ValueError):
        SB.exact_eer([1.0, 2.0], [True, True])
    with pytest.raises(ValueError, match="NaN"):
        SB.exact_eer([1.0, np.nan], [True, False])


def test_the_gpu_cases_keep_the_edges_clear():
    """What tests/test_spk_gpu.py rests on, from the oracle alone: at no edge do more than 0.25 % of a class's trials lie within
    delta of it, for every committed case; and the sweep is the issue's."""
    for name in SC.NAMES:
        c = SC.case(name)
        for cls, (near, total) in enumerate(SC.worst_edge(c)):
            print("%s class %d: at most %d of %d trials within delta of one edge" % (name, cls, near, total))
            assert near <= SC.CAP * total, (name, cls)
    specs = SC.SPECS.values()
    assert {s["S"] for s in specs} == {1, 2, 63, 64, 65, 255, 256, 257, 777, 1100}
    assert {s["width"] for s in specs} == {1, 5, 16, 24, 32, 100, 128}
    assert {s["NB"] for s in specs} == {64, 256, 4096, 8192} and {s["ln"] for s in specs} == {False, True}


def test_oracle_edge_counts_by_hand():
    s = np.array([0.1, 0.5, 0.5, 1.9, 2.0])
    cum, near, hist = R.edge_counts(s, np.array([0.0, 0.01, 0.0, 0.2, 0.0]), 0.0, 2.0, 4)
    assert hist.tolist() == [1, 2, 0, 2] and cum.tolist() == [5, 4, 2, 2, 0]
    # both 0.5 sit on edge 1 (|s - edge| <= delta holds with delta 0); 1.9 touches only the outer edge, which is exact
    assert near.tolist() == [0, 2, 0, 0, 0]
    assert R.edge_counts(s + 0.005, np.array([0.0, 0.01, 0.0, 0.2, 0.0]), 0.0, 2.0, 4)[1].tolist() == [0, 1, 0, 0, 0]
    cum, near, hist = R.edge_counts(s, np.zeros(5), 1.0, 1.0, 4)
    assert hist.tolist() == [5, 0, 0, 0] and not near.any()


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_signatures_match_the_header():
    import hip_binding as hb
    import spk_backend as SB

    text = ext_abi.header_text("fhvae_spk.h")
    found = ext_abi.declared("fhvae_spk.h", "fhvae_spk_")
    assert found == SB.SPK_SIGNATURES
    assert sorted(found) == ["fhvae_spk_llr_hist", "fhvae_spk_llr_range", "fhvae_spk_llr_trials", "fhvae_spk_project", "fhvae_spk_ws_bytes"]
    assert not set(found) & set(hb.SIGNATURES)
    assert int(re.search(r"#define FHVAE_SPK_MAX_IN (\d+)", text).group(1)) == SB.SPK_MAX_IN
    assert int(re.search(r"#define FHVAE_SPK_MAX_ROWS (\d+)", text).group(1)) == SB.SPK_MAX_ROWS == 1 << 24
    for name, value in (("FHVAE_SPK_NAN", SB.SPK_NAN), ("FHVAE_SPK_BAD_INDEX", SB.SPK_BAD_INDEX)):
        assert int(re.search(r"%s = (\d+)" % name, text).group(1)) == value


def test_symbols_exported_and_the_main_header_untouched(lib):
    import hip_binding as hb
    import spk_backend as SB

    for name in SB.SPK_SIGNATURES:
        assert hasattr(lib, name) and name not in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12 and len(hb.SIGNATURES) == 81  # include/fhvae_hip.h is untouched
    assert "fhvae_spk_" not in open(os.path.join(ROOT, "include", "fhvae_hip.h")).read().lower()


def test_workspace_is_positive_and_monotone(lib):
    f = lib.fhvae_spk_ws_bytes
    for D in (16, 32, 48, 64, 80, 96, 112, 128):
        last = 0
        for S in (1, 2, 255, 256, 257, 28000, 100000, 1 << 24):
            got = f(S, D)
            assert got > 0 and got >= last and got % 256 == 0, (S, D)
            last = got
    for bad in ((0, 32), (-1, 32), ((1 << 24) + 1, 32), (10, 8), (10, 0), (10, 40), (10, 144)):
        assert f(*bad) == 0, bad


def test_project_errors_before_any_launch(lib):
    keep, p = ext_abi.aligned()
    fn = lib.fhvae_spk_project
    #       x ldx S  Din A lda K mean normalise q scale out ldo a stream
    good = [p, 24, 5, 24, p, 24, 16, p, 1, p, p, p, 16, p, None]
    for i in (0, 4, 7, 11):
        assert fn(*_swap(good, i, None)) == NULL, i
    assert fn(*_swap(good, 9, None)) == NULL and fn(*_swap(good, 13, None)) == NULL  # (q and a come together)
    for i, bad in ((2, 0), (2, -1), (3, 0), (6, 0), (6, 129), (1, 23), (5, 23), (12, 15), (12, 12), (12, 18)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i, bad in ((0, p + 2), (4, p + 1), (7, p + 2), (9, p + 2), (10, p + 3), (13, p + 2), (11, p + 4), (11, p + 8)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    assert fn(*_swap(_swap(_swap(good, 3, 1025), 1, 1025), 5, 1025)) == LIMIT
    assert fn(*_swap(good, 2, (1 << 24) + 1)) == LIMIT
    del keep


def _scoring_errors(fn, good, ptrs, S_at, D_at, ld_at):
    for i in ptrs:
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((S_at, 0), (S_at, -1), (D_at, 8), (D_at, 40), (D_at, 144), (D_at, 0), (ld_at, 28)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    assert fn(*_swap(good, ld_at, 34)) == ALIGN and fn(*_swap(good, 0, good[0] + 4)) == ALIGN
    assert fn(*_swap(good, S_at, (1 << 24) + 1)) == LIMIT


def test_range_errors_before_any_launch(lib):
    keep, p = ext_abi.aligned()
    fn = lib.fhvae_spk_llr_range
    #       v ld a label S  D  c    ws ws_bytes range status stream
    good = [p, 32, p, p, 10, 32, 0.5, p, 256, p, p, None]
    _scoring_errors(fn, good, (0, 2, 3, 7, 9, 10), 4, 5, 1)
    assert fn(*_swap(good, 8, 255)) == SHAPE and fn(*_swap(good, 8, 0)) == SHAPE
    for i in (2, 3, 7, 9, 10):
        assert fn(*_swap(good, i, p + 2)) == ALIGN, i
    del keep


def test_hist_errors_before_any_launch(lib):
    keep, p = ext_abi.aligned()
    fn = lib.fhvae_spk_llr_hist
    #       v ld a label S  D  c    lo   hi   NB hist status stream
    good = [p, 32, p, p, 10, 32, 0.5, -3.0, 4.0, 256, p, p, None]
    _scoring_errors(fn, good, (0, 2, 3, 10, 11), 4, 5, 1)
    for bad in (32, 63, 100, 16384, 0, -64):
        assert fn(*_swap(good, 9, bad)) == SHAPE, bad
    for i, bad in ((7, float("nan")), (7, float("-inf")), (8, float("inf")), (8, float("nan")), (8, -3.5)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i, bad in ((2, p + 2), (3, p + 2), (10, p + 4), (11, p + 2)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    del keep


def test_trials_errors_before_any_launch(lib):
    keep, p = ext_abi.aligned()
    fn = lib.fhvae_spk_llr_trials
    #       v ld a  S  D  c    pairs n out status stream
    good = [p, 32, p, 10, 32, 0.5, p, 7, p, p, None]
    _scoring_errors(fn, good, (0, 2, 6, 8, 9), 3, 4, 1)
    assert fn(*_swap(good, 7, 0)) == SHAPE and fn(*_swap(good, 7, -2)) == SHAPE
    assert fn(*_swap(good, 7, 1 << 31)) == LIMIT
    for i in (2, 6, 8, 9):
        assert fn(*_swap(good, i, p + 2)) == ALIGN, i
    del keep


def test_calls_refuse_cpu_tensors():
    import spk_backend as SB

    v, a, lab = torch.zeros(4, 16), torch.zeros(4), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensor"):
        SB.project(v, torch.eye(16), torch.zeros(16))
    with pytest.raises(RuntimeError, match="device tensor"):
        SB.llr_range(v, a, lab, 0.0)
    with pytest.raises(RuntimeError, match="device tensor"):
        SB.llr_hist(v, a, lab, 0.0, -1.0, 1.0)
    with pytest.raises(RuntimeError, match="device tensor"):
        SB.llr_trials(v, a, 0.0, torch.zeros(2, 2, dtype=torch.int32))


# --------------------------------------------------------------------------------------------------------------------- CLI
def _stub_gpu(monkeypatch):
    """Everything that needs a device, replaced by the oracle: all-pairs cosine and the back end's two scorings."""
    import spk_backend as SB
    import verification as V

    def hist_of(s, same, lo, hi, NB):
        h = np.zeros((2, NB), dtype=np.int64)
        w = (hi - lo) / NB
        b = np.clip(np.floor((s - lo) / w), 0, NB - 1).astype(np.int64) if hi > lo else np.zeros(len(s), np.int64)
        np.add.at(h[0], b[same], 1)
        np.add.at(h[1], b[~same], 1)
        return h

    def speaker_verification(emb, labels, n_bins=4096, device=None):
        e = emb.cpu().numpy() if isinstance(emb, torch.Tensor) else np.asarray(emb)
        i, j, same = R.trials(np.asarray(labels))
        hist = hist_of(R.cosine_scores(e, i, j), same, -1.0, 1.0, n_bins)
        return dict(V.eer_from_hist(hist), hist=hist)

    def score_all_pairs(self, emb, labels, n_bins=4096, lo=None, hi=None, backend="plda", dcf=(0.01, 1.0, 1.0), device=None):
        e = emb.cpu().numpy() if isinstance(emb, torch.Tensor) else np.asarray(emb)
        i, j, same = R.trials(np.asarray(labels))
        tab = self.tables_f32()
        if backend == "lda":
            y = R.project(e, tab["A1"], tab["m"], normalise=self.length_norm)[0]
            s, lo, hi = R.cosine_scores(y, i, j), -1.0, 1.0
        else:
            v, a = R.transform32(tab, e, self.length_norm)
            s, _ = R.scores(v, a, tab["c"], i, j)
            lo, hi = float(s.min()), float(s.max())
        hist = hist_of(s, same, lo, hi, n_bins)
        return dict(SB.eer_from_hist(hist, lo, hi, dcf), hist=hist)

    def score_trials(self, emb, pairs, device=None):
        tab = self.tables_f32()
        v, a = R.transform32(tab, np.asarray(emb), self.length_norm)
        p = np.asarray(pairs)
        return R.scores(v, a, tab["c"], p[:, 0], p[:, 1])[0].astype(np.float32)

    monkeypatch.setattr(V, "speaker_verification", speaker_verification)
    monkeypatch.setattr(SB.Backend, "score_all_pairs", score_all_pairs)
    monkeypatch.setattr(SB.Backend, "score_trials", score_trials)


def _archives(tmp_path):
    """A training archive in the numpy form and an evaluation archive in the Kaldi form (one-row matrices), keys <spk>-<n>."""
    import kaldi_io_lite as K

    x, label = R.planted(21, 12, 8, 8, nuisance=3.0)
    xe, le = R.planted(22, 6, 6, 8, nuisance=3.0)
    train, ev = tmp_path / "train", tmp_path / "eval"
    train.mkdir(), ev.mkdir()
    np.save(train / "mu2.npy", x)
    tkeys = ["t%02d-%d" % (s, n) for n, s in enumerate(label)]
    (train / "keys.txt").write_text("".join(k + "\n" for k in tkeys))
    ekeys = ["e%02d-%d" % (s, n) for n, s in enumerate(le)]
    K.write_ark_scp(str(ev / "feats.ark"), str(ev / "feats.scp"), [(k, r[None, :]) for k, r in zip(ekeys, xe)])
    return str(train), str(ev), ekeys, xe, le


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_score_speakers_command_line(tmp_path, monkeypatch, capsys):
    import score_speakers as SS
    import spk_backend as SB

    _stub_gpu(monkeypatch)
    train, ev, ekeys, xe, le = _archives(tmp_path)
    keys, rows = SS.read_archive(ev)
    assert keys == ekeys and np.array_equal(rows, xe)  # (the Kaldi form gives back the rows)
    trials = tmp_path / "trials"
    trials.write_text("%s %s target\n\n%s %s nontarget\n%s %s %s\n" % (
        ekeys[0], ekeys[0], ekeys[0], ekeys[1], ekeys[2], ekeys[3], "target" if le[2] == le[3] else "nontarget"))
    out = tmp_path / "out"
    base = ["--eval-emb", ev, "--spk-key-sep", "-", "--bins", "64"]
    assert SS.main(base + ["--train-emb", train, "--backend", "plda", "cosine", "lda", "--lda-dim", "4", "--trials", str(trials),
                           "--out", str(out)]) == 0
    report = json.loads(capsys.readouterr().out)
    assert report == json.load(open(out / "speakers.json"))
    assert sorted(os.listdir(out)) == ["backend.npz", "hist_cosine.npy", "hist_lda.npy", "hist_plda.npy", "scores.txt", "speakers.json"]
    assert list(report) == ["sequences", "speakers", "unlabelled", "bins", "cosine", "lda", "plda"]
    assert (report["sequences"], report["speakers"], report["unlabelled"], report["bins"]) == (len(ekeys), 6, 0, 64)
    n = len(ekeys)
    for name in ("cosine", "lda", "plda"):
        b = report[name]
        assert set(b) >= {"eer", "threshold", "min_dcf", "crossing_mass", "n_target", "n_nontarget", "lo", "hi"}
        assert b["n_target"] + b["n_nontarget"] == n * (n - 1) // 2 and 0.0 <= b["eer"] <= 1.0 and b["lo"] <= b["threshold"] <= b["hi"]
        h = np.load(out / ("hist_%s.npy" % name))
        assert h.shape == (2, 64) and h[0].sum() == b["n_target"] and h[1].sum() == b["n_nontarget"]
    assert (report["cosine"]["lo"], report["cosine"]["hi"]) == (-1.0, 1.0) and report["plda"]["eer"] < report["cosine"]["eer"]
    assert set(report["plda"]["trials"]) == {"eer", "threshold", "n_target", "n_nontarget"}
    lines = (out / "scores.txt").read_text().splitlines()
    assert [ln.split()[:2] for ln in lines] == [[ekeys[0], ekeys[0]], [ekeys[0], ekeys[1]], [ekeys[2], ekeys[3]]]
    # the model file gives the same figures without the training archive
    again = tmp_path / "again"
    assert SS.main(base + ["--model", str(out / "backend.npz"), "--backend", "plda", "--out", str(again)]) == 0
    capsys.readouterr()
    assert json.load(open(again / "speakers.json"))["plda"] == {k: v for k, v in report["plda"].items() if k != "trials"}
    be = SB.Backend.load(str(out / "backend.npz"))
    assert be.A_lda.shape == (4, 8) and be.length_norm
    # cosine alone trains nothing and writes no model
    plain = tmp_path / "plain"
    assert SS.main(base + ["--out", str(plain)]) == 0
    capsys.readouterr()
    assert sorted(os.listdir(plain)) == ["hist_cosine.npy", "speakers.json"]


def test_score_speakers_errors_name_the_line_or_the_key(tmp_path, monkeypatch, capsys):
    import kaldi_io_lite as K
    import score_speakers as SS

    _stub_gpu(monkeypatch)
    train, ev, ekeys, xe, _ = _archives(tmp_path)
    for text, want in (("%s %s maybe\n" % (ekeys[0], ekeys[1]), r"trials:1: expected"), ("%s target\n" % ekeys[0], r"trials:1: expected"),
                       ("%s %s target\n%s nobody target\n" % (ekeys[0], ekeys[1], ekeys[0]), r"trials:2: key 'nobody'"), ("\n", "no trial")):
        (tmp_path / "trials").write_text(text)
        with pytest.raises(ValueError, match=want):
            SS.read_trials(str(tmp_path / "trials"), ekeys)
    # an archive entry with two rows, and one of another width: the line and the key
    K.write_ark_scp(str(tmp_path / "two.ark"), str(tmp_path / "two.scp"), [("a-1", xe[:1]), ("b-1", xe[:2])])
    with pytest.raises(ValueError, match=r"two.scp:2: key 'b-1' holds a matrix of shape \(2, 8\)"):
        SS.read_archive(str(tmp_path / "two.scp"))
    K.write_ark_scp(str(tmp_path / "w.ark"), str(tmp_path / "w.scp"), [("a-1", xe[:1]), ("b-1", xe[:1, :5])])
    with pytest.raises(ValueError, match=r"w.scp:2: key 'b-1' has 5 columns"):
        SS.read_archive(str(tmp_path / "w.scp"))
    K.write_ark_scp(str(tmp_path / "d.ark"), str(tmp_path / "d.scp"), [("a-1", xe[:1]), ("a-1", xe[1:2])])
    with pytest.raises(ValueError, match="key 'a-1' is listed twice"):
        SS.read_archive(str(tmp_path / "d.scp"))
    # vectors (an i-vector archive) are read too
    K.write_vec_ark_scp(str(tmp_path / "v.ark"), str(tmp_path / "v.scp"), [("a-1", xe[0]), ("b-1", xe[1])])
    keys, rows = SS.read_archive(str(tmp_path / "v.scp"))
    assert keys == ["a-1", "b-1"] and np.array_equal(rows, xe[:2])
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="neither"):
        SS.read_archive(str(tmp_path / "empty"))
    # the command line: the message reaches stderr, the exit code is 1; flag errors exit with 2
    (tmp_path / "trials").write_text("%s nobody target\n" % ekeys[0])
    assert SS.main(["--eval-emb", ev, "--train-emb", train, "--spk-key-sep", "-", "--backend", "plda", "--trials", str(tmp_path / "trials"),
                    "--out", str(tmp_path / "o")]) == 1
    assert "trials:1: key 'nobody'" in capsys.readouterr().err
    for extra in (["--backend", "plda"], ["--backend", "lda", "--train-emb", train], ["--bins", "100"],
                  ["--backend", "plda", "--train-emb", train, "--model", "m.npz"]):
        with pytest.raises(SystemExit) as e:
            SS.parse_args(["--eval-emb", ev, "--spk-key-sep", "-", "--out", "o"] + extra)
        assert e.value.code == 2, extra
    capsys.readouterr()


def test_eval_model_outputs_with_and_without_the_back_end(tmp_path, monkeypatch, capsys):
    import eval_model as EM

    _stub_gpu(monkeypatch)
    xe, le = R.planted(31, 6, 6, 8, nuisance=3.0)
    xt, lt = R.planted(32, 12, 8, 8, nuisance=3.0)
    keys = ["e%02d-%d" % (s, n) for n, s in enumerate(le)]
    tkeys = ["t%02d-%d" % (s, n) for n, s in enumerate(lt)]
    z1 = np.repeat(xe[:, ::-1], 2, axis=0).astype(np.float32)  # (two segments per sequence)
    seq_pos = np.repeat(np.arange(len(keys)), 2)
    monkeypatch.setattr(EM, "sv_train_embeddings", lambda args, model, T, dev: (tkeys, {"mu2": xt, "z1_mean": xt[:, ::-1].copy()}))
    base = ["--checkpoint", "c.tar", "--feat-scp", "f.scp", "--len-scp", "l.scp", "--spk-key-sep", "-", "--sv-bins", "64"]
    train = ["--sv-train-feat-scp", "t.scp", "--sv-train-len-scp", "t.len"]
    got = {}
    for name, extra in (("plain", []), ("cosine", ["--sv-backend", "cosine"]),
                        ("both", ["--sv-backend", "cosine", "lda", "plda", "--sv-lda-dim", "4", "--sv-plda-iters", "3"] + train),
                        ("plda", ["--sv-backend", "plda", "--sv-no-length-norm"] + train)):
        d = tmp_path / name
        d.mkdir()
        args = EM.parse_args(base + ["--out", str(d)] + extra)
        tr = EM.sv_train_embeddings(args, None, 20, None) if args.sv_trained else None
        got[name] = (EM.verify_speakers(args, keys, xe, z1, seq_pos, str(d), torch.device("cpu"), tr), _files(str(d)))
    # without --sv-backend, or with cosine alone: what it is today, byte for byte
    assert json.dumps(got["plain"][0]) == json.dumps(got["cosine"][0]) and got["plain"][1] == got["cosine"][1]
    assert sorted(got["plain"][1]) == ["sv_hist_mu2.npy", "sv_hist_z1_mean.npy"]
    assert set(got["plain"][0]["mu2"]) == {"eer", "threshold", "n_target", "n_nontarget", "crossing_mass"}
    # with it: the same entries and files, and the new ones beside them
    block, files = got["both"]
    assert sorted(files) == sorted(list(got["plain"][1]) + ["sv_backend_%s.npz" % n for n in ("mu2", "z1_mean")]
                                   + ["sv_hist_%s_%s.npy" % (n, b) for n in ("mu2", "z1_mean") for b in ("lda", "plda")])
    assert all(files[f] == got["plain"][1][f] for f in got["plain"][1])
    for name in ("mu2", "z1_mean"):
        entry = dict(block[name])
        lda, plda = entry.pop("lda"), entry.pop("plda")
        assert entry == got["plain"][0][name]
        for b in (lda, plda):
            assert set(b) == {"eer", "threshold", "min_dcf", "crossing_mass", "n_target", "n_nontarget", "lo", "hi"}
            assert b["n_target"] == entry["n_target"] and b["n_nontarget"] == entry["n_nontarget"]
    assert {k: v for k, v in block.items() if k not in ("mu2", "z1_mean")} == {k: v for k, v in got["plain"][0].items() if k not in ("mu2", "z1_mean")}
    assert block["mu2"]["plda"]["eer"] < block["mu2"]["eer"]
    assert set(got["plda"][0]["mu2"]) == set(got["plain"][0]["mu2"]) | {"plda"}
    json.dumps(block)  # (the block goes into summary.json)
    # flag errors
    for extra in (["--sv-backend", "plda"], ["--sv-backend", "lda"] + train, ["--sv-lda-dim", "4"], ["--sv-train-feat-scp", "t.scp"],
                  ["--sv-backend", "plda", "--sv-plda-iters", "-1"] + train):
        with pytest.raises(SystemExit) as e:
            EM.parse_args(base + ["--out", "o"] + extra)
        assert e.value.code == 2, extra
    with pytest.raises(SystemExit):
        EM.parse_args(["--checkpoint", "c.tar", "--feat-scp", "f.scp", "--len-scp", "l.scp", "--out", "o", "--sv-backend", "plda"] + train)
    capsys.readouterr()
