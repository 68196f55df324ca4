"""Score normalisation without a GPU: the oracle's own claims (affine invariance, S-norm as the z-norm / t-norm average, the
Lipschitz bounds the GPU tests rest on), the two conditions those tests need (clear histogram edges on every committed case, an
effect on the two-condition set), the header against the module's table, every argument error of the five calls, make_cohort, and
both command lines with the GPU part replaced by the oracle."""
import json
import os
import re

import numpy as np
import pytest
import torch

import ext_abi
import snorm_cases as NC
import snorm_ref as N
import spk_cases as SC
import spk_ref as R
import test_spk_cpu as TS
from ext_abi import swap as _swap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, ALIGN, LIMIT = -1, -2, -4, -5


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import score_norm

    return score_norm.load_library()


@pytest.fixture(scope="module")
def two():
    """The two-condition set through the oracle's f32 transform: per back end (v, a, z, az, c), and the trials."""
    d = N.two_conditions()
    tab = R.tables(d["model"])
    i, j, same = R.trials(d["label"])
    rows = {"plda": R.transform32(tab, d["x"], True) + R.transform32(tab, d["cohort"], True) + (tab["c"],),
            "cosine": N.unit_rows(d["x"]) + N.unit_rows(d["cohort"]) + (0.0,)}
    return rows, i, j, same


# ---------------------------------------------------------------------------------------------------------------- the oracle
def test_the_normalised_score_is_affine_invariant(two):
    rows, i, j, same = two
    v, a, z, az, c = rows["plda"]
    s, _ = R.scores(v, a, c, i, j)
    cs, _ = N.cohort_scores(v, a, z, az, c)
    for top in (0, 200, 1 + 1):
        _, mu, sd = N.stats(cs, top)
        base = N.normalise(s, mu, 1.0 / sd, i, j)
        for alpha, beta in ((3.5, -7.0), (0.01, 100.0)):
            _, mu2, sd2 = N.stats(alpha * cs + beta, top)
            moved = N.normalise(alpha * s + beta, mu2, 1.0 / sd2, i, j)
            assert np.abs(moved - base).max() <= 1e-9 * max(1.0, np.abs(base).max())
    # mu = 0, r = 1: the score itself
    assert np.array_equal(N.normalise(s, np.zeros(len(v)), np.ones(len(v)), i, j), 0.5 * (s + s))


def test_the_whole_cohort_gives_the_average_of_z_norm_and_t_norm(two):
    rows, i, j, same = two
    v, a, z, az, c = rows["cosine"]
    s, _ = R.scores(v, a, c, i, j)
    cs, _ = N.cohort_scores(v, a, z, az, c)
    _, mu, sd = N.stats(cs, 0)
    znorm = (s - cs.mean(axis=1)[i]) / cs.std(axis=1)[i]
    tnorm = (s - cs.mean(axis=1)[j]) / cs.std(axis=1)[j]
    assert np.abs(N.normalise(s, mu, 1.0 / sd, i, j) - 0.5 * (znorm + tnorm)).max() <= 1e-9
    assert N.top_k(0, 600) == N.top_k(-3, 600) == N.top_k(600, 600) == N.top_k(605, 600) == 600 and N.top_k(20, 600) == 20


def test_order_statistics_mean_and_deviation_are_lipschitz():
    rs = np.random.RandomState(3)
    for S, Nc, top in ((40, 1, 0), (40, 2, 1), (60, 17, 5), (30, 200, 0), (30, 200, 199), (30, 200, 20)):
        s = rs.randn(S, Nc) * rs.uniform(0.1, 10.0, size=(S, 1))
        s[:, ::3] = np.round(s[:, ::3])  # (ties)
        thr, mu, sd = N.stats(s, top)
        for eps in (1e-6, 1e-2, 1.0):
            for _ in range(5):
                p = s + eps * rs.uniform(-1.0, 1.0, size=s.shape) * (rs.rand(*s.shape) < 0.7)
                t2, m2, d2 = N.stats(p, top)
                slack = 1e-12 * (1.0 + np.abs(s).max())
                assert (np.abs(t2 - thr) <= eps + slack).all() and (np.abs(m2 - mu) <= eps + slack).all() and (np.abs(d2 - sd) <= eps + slack).all()
    # by hand
    thr, mu, sd = N.stats(np.array([[1.0, 5.0, 3.0, 3.0, -2.0]]), 3)
    assert (thr[0], mu[0]) == (3.0, 11.0 / 3.0) and abs(sd[0] - np.sqrt(8.0 / 9.0)) < 1e-15


def test_the_gpu_cases_keep_the_edges_clear():
    """What tests/test_snorm_gpu.py rests on, from the oracle alone: at no histogram edge do more than 0.25 % of a class's trials
    lie within Delta of it, at the case's NB and at every NB from 64 to 8192 for the largest case; and the sweep is the issue's."""
    for name in NC.PAIRS_NAMES:
        c = SC.case(name)
        mu, r = NC.oracle_stats(name)
        lo, hi = NC.score_range(c, mu, r)
        for NB in sorted({c["NB"]} | ({64, 128, 256, 512, 1024, 2048, 4096, 8192} if name == "S777-w24" else set())):
            for cls, (s, _, _, near, _) in enumerate(NC.classes(c, mu, r, lo, hi, NB)):
                worst = int(near.max()) if len(s) else 0
                print("%s NB %d class %d: at most %d of %d trials within Delta of one edge" % (name, NB, cls, worst, len(s)))
                assert worst <= SC.CAP * len(s), (name, NB, cls)
    specs = NC.STATS.values()
    assert {s["S"] for s in specs} == {1, 63, 64, 65, 255, 256, 257, 600}
    assert {s["Nc"] for s in specs} == {1, 2, 15, 16, 17, 63, 64, 65, 129, 1000}
    assert {s["width"] for s in specs} == {1, 5, 16, 24, 48, 100, 128}
    assert {0, 1, 2, 20} <= {s["top"] for s in specs} and {s["top"] - s["Nc"] for s in specs} >= {-1, 0, 5}
    for kind in NC.EXACT_KINDS:
        v, a, z, az, c, top = NC.exact_case(kind)
        s, _ = N.cohort_scores(v, a, z, az, c)
        assert np.array_equal(s, np.round(s)) and np.abs(s).max() < 2 ** 20


def test_normalisation_helps_on_the_two_conditions(two):
    """The PLDA fitted on one condition: the oracle's normalised EER is at most 0.9 of its raw EER for top 0 and top 200 (0.68
    and 0.77 here).  The raw cosine gains less on this set (0.90): it is held to `below the raw EER`, what the GPU test asks."""
    rows, i, j, same = two
    for which, need in (("plda", 0.9), ("cosine", 1.0)):
        v, a, z, az, c = rows[which]
        s, _ = R.scores(v, a, c, i, j)
        raw = R.exact_eer(s[same], s[~same])
        cs, _ = N.cohort_scores(v, a, z, az, c)
        for top in (0, 200):
            _, mu, sd = N.stats(cs, top)
            sn = N.normalise(s, mu, 1.0 / sd, i, j)
            eer = R.exact_eer(sn[same], sn[~same])
            print("%s top %d: EER %.4f, raw %.4f, ratio %.3f" % (which, top, eer, raw, eer / raw))
            assert eer < need * raw if need == 1.0 else eer <= need * raw


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_signatures_match_the_header():
    import hip_binding as hb
    import score_norm as SN

    text = ext_abi.header_text("fhvae_snorm.h")
    found = ext_abi.declared("fhvae_snorm.h", "fhvae_sn_")
    assert found == SN.SN_SIGNATURES
    assert sorted(found) == ["fhvae_sn_cohort_stats", "fhvae_sn_hist", "fhvae_sn_range", "fhvae_sn_trials", "fhvae_sn_ws_bytes"]
    assert not set(found) & set(hb.SIGNATURES)
    assert int(re.search(r"#define FHVAE_SN_MAX_ROWS (\d+)", text).group(1)) == SN.SN_MAX_ROWS == 1 << 24
    assert int(re.search(r"#define FHVAE_SN_MAX_COHORT (\d+)", text).group(1)) == SN.SN_MAX_COHORT == 1 << 20
    for name, value in (("FHVAE_SN_NAN", SN.SN_NAN), ("FHVAE_SN_BAD_INDEX", SN.SN_BAD_INDEX), ("FHVAE_SN_NONFINITE", SN.SN_NONFINITE)):
        assert int(re.search(r"%s = (\d+)" % name, text).group(1)) == value


def test_symbols_exported_and_the_main_header_untouched(lib):
    import hip_binding as hb
    import score_norm as SN

    for name in SN.SN_SIGNATURES:
        assert hasattr(lib, name) and name not in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12 and len(hb.SIGNATURES) == 81
    assert "fhvae_sn_" not in open(os.path.join(ROOT, "include", "fhvae_hip.h")).read().lower()
    for S, D in ((1, 16), (257, 32), (1 << 24, 128)):
        assert lib.fhvae_sn_ws_bytes(S, D) == lib.fhvae_spk_ws_bytes(S, D) > 0
    for bad in ((0, 32), ((1 << 24) + 1, 32), (10, 8), (10, 40), (10, 144)):
        assert lib.fhvae_sn_ws_bytes(*bad) == 0, bad


def test_cohort_stats_errors_before_any_launch(lib):
    keep, p = ext_abi.aligned()
    fn = lib.fhvae_sn_cohort_stats
    #       v ld a  S  z ldz az Nc  D  c   top sd_floor mu sd r thr status stream
    good = [p, 32, p, 10, p, 32, p, 7, 32, 0.5, 3, 1e-6, p, p, p, p, p, None]
    assert fn(*_swap(good, 11, float("nan"))) == SHAPE  # (the list itself is never launched: every call below changes one argument)
    for i in (0, 2, 4, 6, 12, 13, 14, 15, 16):
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((3, 0), (3, -1), (7, 0), (7, -5), (8, 8), (8, 40), (8, 144), (8, 0), (1, 28), (5, 28), (11, 0.0), (11, -1.0),
                   (11, float("inf")), (11, float("nan"))):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i, bad in ((1, 34), (5, 34), (0, p + 4), (4, p + 8), (2, p + 2), (6, p + 2), (12, p + 1), (13, p + 2), (14, p + 3), (15, p + 2), (16, p + 2)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    assert fn(*_swap(good, 3, (1 << 24) + 1)) == LIMIT and fn(*_swap(good, 7, (1 << 20) + 1)) == LIMIT
    del keep


def _scoring_errors(fn, good, ptrs, aligned4, S_at, D_at, ld_at):
    for i in ptrs:
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((S_at, 0), (S_at, -1), (D_at, 8), (D_at, 40), (D_at, 144), (D_at, 0), (ld_at, 28)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    assert fn(*_swap(good, ld_at, 34)) == ALIGN and fn(*_swap(good, 0, good[0] + 4)) == ALIGN
    for i in aligned4:
        assert fn(*_swap(good, i, good[0] + 2)) == ALIGN, i
    assert fn(*_swap(good, S_at, (1 << 24) + 1)) == LIMIT


def test_range_hist_and_trials_errors_before_any_launch(lib):
    keep, p = ext_abi.aligned()
    #       v ld a mu r label S  D  c    ws ws_bytes range status stream
    good = [p, 32, p, p, p, p, 10, 32, 0.5, p, 256, p, p, None]
    _scoring_errors(lib.fhvae_sn_range, good, (0, 2, 3, 4, 5, 9, 11, 12), (2, 3, 4, 5, 9, 11, 12), 6, 7, 1)
    assert lib.fhvae_sn_range(*_swap(good, 10, 255)) == SHAPE and lib.fhvae_sn_range(*_swap(good, 10, 0)) == SHAPE
    #       v ld a mu r label S  D  c    lo   hi   NB hist status stream
    good = [p, 32, p, p, p, p, 10, 32, 0.5, -3.0, 4.0, 256, p, p, None]
    fn = lib.fhvae_sn_hist
    _scoring_errors(fn, good, (0, 2, 3, 4, 5, 12, 13), (2, 3, 4, 5, 13), 6, 7, 1)
    for bad in (32, 63, 100, 16384, 0, -64):
        assert fn(*_swap(good, 11, bad)) == SHAPE, bad
    for i, bad in ((9, float("nan")), (9, float("-inf")), (10, float("inf")), (10, float("nan")), (10, -3.5)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    assert fn(*_swap(good, 12, p + 4)) == ALIGN
    #       v ld a mu r  S  D  c    pairs n out status stream
    good = [p, 32, p, p, p, 10, 32, 0.5, p, 7, p, p, None]
    fn = lib.fhvae_sn_trials
    _scoring_errors(fn, good, (0, 2, 3, 4, 8, 10, 11), (2, 3, 4, 8, 10, 11), 5, 6, 1)
    assert fn(*_swap(good, 9, 0)) == SHAPE and fn(*_swap(good, 9, -2)) == SHAPE and fn(*_swap(good, 9, 1 << 31)) == LIMIT
    del keep


def test_calls_refuse_cpu_tensors_and_bad_arguments():
    import score_norm as SN

    v, a, lab = torch.zeros(4, 16), torch.zeros(4), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensor"):
        SN.cohort_stats(v, a, v, a, 0.0)
    with pytest.raises(RuntimeError, match="device tensor"):
        SN.norm_range(v, a, a, a, lab, 0.0)
    with pytest.raises(RuntimeError, match="device tensor"):
        SN.norm_hist(v, a, a, a, lab, 0.0, -1.0, 1.0)
    with pytest.raises(RuntimeError, match="device tensor"):
        SN.norm_trials(v, a, a, a, 0.0, torch.zeros(2, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="which"):
        SN.operands(None, v, "psda")


def test_make_cohort():
    import score_norm as SN

    x = np.arange(24, dtype=np.float64).reshape(8, 3)
    lab = np.array([2, 0, 2, -1, 0, 5, 2, -1])
    means = SN.make_cohort(x, lab)
    assert means.dtype == np.float32 and means.shape == (3, 3)
    assert np.array_equal(means, np.stack([x[[1, 4]].mean(0), x[[0, 2, 6]].mean(0), x[5]]).astype(np.float32))
    assert np.array_equal(SN.make_cohort(x, lab, "rows"), x[lab >= 0].astype(np.float32))
    assert np.array_equal(SN.make_cohort(torch.from_numpy(x), None, "rows"), x.astype(np.float32))
    sub = SN.make_cohort(x, None, "rows", max_rows=3, seed=1)
    assert sub.shape == (3, 3) and np.array_equal(sub, SN.make_cohort(x, None, "rows", max_rows=3, seed=1))
    idx = [int(r[0]) // 3 for r in sub]
    assert idx == sorted(idx) and len(set(idx)) == 3
    assert SN.make_cohort(x, lab, max_rows=3).shape == (3, 3)
    for bad in (dict(labels=None), dict(labels=lab[:5]), dict(labels=lab, mode="centroids"), dict(labels=np.full(8, -1))):
        with pytest.raises(ValueError):
            SN.make_cohort(x, **bad)
    with pytest.raises(ValueError, match="finite"):
        SN.make_cohort(np.where(x == 4, np.nan, x), lab)


# --------------------------------------------------------------------------------------------------------------------- CLI
def _stub_snorm(monkeypatch):
    """score_norm's two device paths replaced by the oracle (spk_backend's are replaced by tests/test_spk_cpu.py's stub)."""
    import score_norm as SN
    import spk_backend as SB

    calls = []

    def rows_of(backend, emb, which):
        e = emb.cpu().numpy() if isinstance(emb, torch.Tensor) else np.asarray(emb)
        if which == "cosine":
            return N.unit_rows(e) + (0.0,)
        tab = backend.tables_f32()
        if which == "lda":
            return N.unit_rows(R.project(e, tab["A1"], tab["m"], normalise=backend.length_norm)[0]) + (0.0,)
        return R.transform32(tab, e, backend.length_norm) + (tab["c"],)

    def normalised(backend, emb, cohort_emb, top, which, i, j):
        v, a, c = rows_of(backend, emb, which)
        z, az, _ = rows_of(backend, cohort_emb, which)
        cs, _ = N.cohort_scores(v, a, z, az, c)
        _, mu, sd = N.stats(cs, top)
        return N.normalise(R.scores(v, a, c, i, j)[0], mu, 1.0 / np.maximum(sd, 1e-6), i, j), len(z)

    def score_all_pairs(backend, emb, labels, cohort_emb, top=200, which="plda", n_bins=4096, dcf=(0.01, 1.0, 1.0), sd_floor=1e-6, device=None):
        i, j, same = R.trials(np.asarray(labels))
        s, Nc = normalised(backend, emb, cohort_emb, top, which, i, j)
        lo, hi = float(s.min()), float(s.max())
        hist = np.zeros((2, n_bins), dtype=np.int64)
        b = np.clip(np.floor((s - lo) / ((hi - lo) / n_bins)), 0, n_bins - 1).astype(np.int64)
        np.add.at(hist[0], b[same], 1)
        np.add.at(hist[1], b[~same], 1)
        calls.append((which, top, Nc))
        return dict(SB.eer_from_hist(hist, lo, hi, dcf), hist=hist, top=N.top_k(top, Nc), cohort=Nc)

    def score_trials(backend, emb, pairs, cohort_emb, top=200, which="plda", sd_floor=1e-6, device=None):
        p = np.asarray(pairs)
        return normalised(backend, emb, cohort_emb, top, which, p[:, 0], p[:, 1])[0].astype(np.float32)

    monkeypatch.setattr(SN, "score_all_pairs", score_all_pairs)
    monkeypatch.setattr(SN, "score_trials", score_trials)
    return calls


FIGURES = {"eer", "threshold", "min_dcf", "crossing_mass", "n_target", "n_nontarget", "lo", "hi"}


def test_score_speakers_command_line(tmp_path, monkeypatch, capsys):
    import score_speakers as SS

    TS._stub_gpu(monkeypatch)
    calls = _stub_snorm(monkeypatch)
    train, ev, ekeys, xe, le = TS._archives(tmp_path)
    trials = tmp_path / "trials"
    trials.write_text("%s %s target\n%s %s nontarget\n%s %s %s\n" % (
        ekeys[0], ekeys[0], ekeys[0], ekeys[1], ekeys[2], ekeys[3], "target" if le[2] == le[3] else "nontarget"))
    common = ["--eval-emb", ev, "--spk-key-sep", "-", "--bins", "64", "--train-emb", train, "--backend", "plda", "cosine", "lda", "--lda-dim", "4",
              "--trials", str(trials)]
    plain, normed = tmp_path / "plain", tmp_path / "normed"
    assert SS.main(common + ["--out", str(plain)]) == 0
    before = json.loads(capsys.readouterr().out)
    assert not calls
    assert SS.main(common + ["--out", str(normed), "--snorm", "--snorm-top", "5"]) == 0
    report = json.loads(capsys.readouterr().out)
    assert report == json.load(open(normed / "speakers.json"))
    # without the flags: what it was, byte for byte; with them: the same files and figures, and the new ones beside them
    old, new = TS._files(str(plain)), TS._files(str(normed))
    assert sorted(set(new) - set(old)) == ["hist_cosine_snorm.npy", "hist_lda_snorm.npy", "hist_plda_snorm.npy", "scores_snorm.txt"]
    assert all(new[f] == old[f] for f in old if f != "speakers.json")
    n = len(ekeys)
    for name in ("cosine", "lda", "plda"):
        entry = dict(report[name])
        block = entry.pop("snorm")
        assert entry == before[name]
        assert set(block) == FIGURES | {"top", "cohort"} | ({"trials"} if name == "plda" else set())
        assert (block["top"], block["cohort"]) == (5, 12) and block["n_target"] + block["n_nontarget"] == n * (n - 1) // 2
        h = np.load(normed / ("hist_%s_snorm.npy" % name))
        assert h.shape == (2, 64) and h[0].sum() == block["n_target"] and h[1].sum() == block["n_nontarget"]
    assert {k: v for k, v in report.items() if k not in ("cosine", "lda", "plda")} == {k: v for k, v in before.items() if k not in ("cosine", "lda", "plda")}
    assert sorted(calls) == [("cosine", 5, 12), ("lda", 5, 12), ("plda", 5, 12)]  # (the speakers' means of the training archive)
    lines = (normed / "scores_snorm.txt").read_text().splitlines()
    assert [ln.split()[:2] for ln in lines] == [[ekeys[0], ekeys[0]], [ekeys[0], ekeys[1]], [ekeys[2], ekeys[3]]]
    assert lines != (normed / "scores.txt").read_text().splitlines()
    # another cohort: the evaluation archive's rows, at most 20 of them, the whole cohort per side; the model from the file
    del calls[:]
    rows = tmp_path / "rows"
    assert SS.main(["--eval-emb", ev, "--spk-key-sep", "-", "--bins", "64", "--model", str(plain / "backend.npz"), "--backend", "plda", "--out", str(rows),
                    "--snorm", "--snorm-top", "0", "--snorm-cohort", ev, "--snorm-cohort-mode", "rows", "--snorm-max-cohort", "20"]) == 0
    r = json.loads(capsys.readouterr().out)
    assert calls == [("plda", 0, 20)] and (r["plda"]["snorm"]["top"], r["plda"]["snorm"]["cohort"]) == (20, 20)
    assert sorted(os.listdir(rows)) == ["backend.npz", "hist_plda.npy", "hist_plda_snorm.npy", "speakers.json"]
    # flag errors
    for extra in (["--snorm", "--snorm-top", "-1", "--train-emb", train], ["--snorm"], ["--snorm", "--snorm-max-cohort", "0", "--train-emb", train],
                  ["--snorm", "--snorm-cohort-mode", "means", "--train-emb", train]):
        with pytest.raises(SystemExit) as e:
            SS.parse_args(["--eval-emb", ev, "--spk-key-sep", "-", "--out", "o"] + extra)
        assert e.value.code == 2, extra
    capsys.readouterr()
    # a cohort of another width is named
    wide = tmp_path / "wide"
    wide.mkdir()
    np.save(wide / "mu2.npy", np.zeros((3, 9), np.float32))
    (wide / "keys.txt").write_text("a-1\nb-1\nc-1\n")
    assert SS.main(["--eval-emb", ev, "--spk-key-sep", "-", "--out", str(tmp_path / "o2"), "--snorm", "--snorm-cohort", str(wide)]) == 1
    assert "9 columns" in capsys.readouterr().err


def test_eval_model_outputs_with_and_without_the_flag(tmp_path, monkeypatch, capsys):
    import eval_model as EM

    TS._stub_gpu(monkeypatch)
    calls = _stub_snorm(monkeypatch)
    xe, le = R.planted(31, 6, 6, 8, nuisance=3.0)
    xt, lt = R.planted(32, 12, 8, 8, nuisance=3.0)
    keys = ["e%02d-%d" % (s, n) for n, s in enumerate(le)]
    tkeys = ["t%02d-%d" % (s, n) for n, s in enumerate(lt)]
    z1 = np.repeat(xe[:, ::-1], 2, axis=0).astype(np.float32)
    seq_pos = np.repeat(np.arange(len(keys)), 2)
    monkeypatch.setattr(EM, "sv_train_embeddings", lambda args, model, T, dev: (tkeys, {"mu2": xt, "z1_mean": xt[:, ::-1].copy()}))
    base = ["--checkpoint", "c.tar", "--feat-scp", "f.scp", "--len-scp", "l.scp", "--spk-key-sep", "-", "--sv-bins", "64"]
    train = ["--sv-backend", "cosine", "lda", "plda", "--sv-lda-dim", "4", "--sv-plda-iters", "3", "--sv-train-feat-scp", "t.scp", "--sv-train-len-scp", "t.len"]
    got = {}
    for name, extra in (("plain", train), ("snorm", train + ["--sv-snorm", "--sv-snorm-top", "0"])):
        d = tmp_path / name
        d.mkdir()
        args = EM.parse_args(base + ["--out", str(d)] + extra)
        tr = EM.sv_train_embeddings(args, None, 20, None)
        got[name] = (EM.verify_speakers(args, keys, xe, z1, seq_pos, str(d), torch.device("cpu"), tr), TS._files(str(d)))
        assert bool(calls) == (name == "snorm")
    (before, old), (block, new) = got["plain"], got["snorm"]
    assert sorted(set(new) - set(old)) == sorted("sv_hist_%s_%s_snorm.npy" % (n, b) for n in ("mu2", "z1_mean") for b in ("lda", "plda"))
    assert all(new[f] == old[f] for f in old)
    for name in ("mu2", "z1_mean"):
        for b in ("lda", "plda"):
            entry = dict(block[name][b])
            sn = entry.pop("snorm")
            assert entry == before[name][b] and set(sn) == FIGURES | {"top", "cohort"} and (sn["top"], sn["cohort"]) == (12, 12)
        assert {k: v for k, v in block[name].items() if k not in ("lda", "plda")} == {k: v for k, v in before[name].items() if k not in ("lda", "plda")}
    json.dumps(block)
    for extra in (["--sv-snorm"], ["--sv-snorm-top", "5"], train + ["--sv-snorm", "--sv-snorm-top", "-1"]):
        with pytest.raises(SystemExit) as e:
            EM.parse_args(base + ["--out", "o"] + extra)
        assert e.value.code == 2, extra
    capsys.readouterr()
