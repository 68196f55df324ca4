"""i-vector extraction without a GPU: the model's identities on the oracle, monotone EM, the ABI of include/fhvae_ivector.h, the
argument errors of its entry points, the packed triangle, files, the command line with the device part stubbed, and the two
conditions the GPU tests rest on, proved on the oracle alone."""
import json
import os
import re

import numpy as np
import pytest
import torch

import ext_abi
import ivector_cases as IC
import ivector_ref as R
from ext_abi import swap as _swap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, ALIGN, LIMIT = -1, -2, -4, -5


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import ivector

    return ivector.load_library()


# ---------------------------------------------------------------------------------------------------------------- the model
def _dense_model(seed, C=3, D=2, R_=2, frames=7):
    """One utterance with HARD component assignments, so that the supervector model is a dense Gaussian: x_t = m_c + s_c (Tt_c w
    + e_t), w and e standard normal."""
    rng = np.random.default_rng(seed)
    ubm = {"weights": np.full(C, 1.0 / C), "means": rng.standard_normal((C, D)), "variances": 0.5 + rng.random((C, D))}
    comp = rng.integers(0, C, frames)
    x = rng.standard_normal((frames, D)) * 2.0
    post = np.eye(C)[comp]
    return rng, ubm, comp, x, post


def _dense_gaussian(ubm, comp, T):
    """The stacked frames z = (x_t - m_c) / s_c of the model are N(0, I + B B^T) with B the stacked Tt_c of the frames' components."""
    D = ubm["means"].shape[1]
    return np.concatenate([T[c][:D] for c in comp])


def test_w_is_the_posterior_mean_of_the_dense_gaussian():
    for seed in range(4):
        rng, ubm, comp, x, post = _dense_model(seed)
        C, D = ubm["means"].shape
        T = np.zeros((C, R.padded(D), 2))
        T[:, :D] = rng.standard_normal((C, D, 2))
        n, f, _, _ = R.stats64(x, post, [0, len(x)])
        w, E, _ = R.estep(n, R.whiten(n, f, ubm), T)
        B = _dense_gaussian(ubm, comp, T)
        z = np.concatenate([(x[t] - ubm["means"][c]) / np.sqrt(ubm["variances"][c]) for t, c in enumerate(comp)])
        # E[w | z] = B^T (I + B B^T)^-1 z,  Cov[w | z] = I - B^T (I + B B^T)^-1 B
        S = np.eye(len(z)) + B @ B.T
        assert np.abs(w[0] - B.T @ np.linalg.solve(S, z)).max() < 1e-9
        assert np.abs(E[0] - np.outer(w[0], w[0]) - (np.eye(2) - B.T @ np.linalg.solve(S, B))).max() < 1e-9


def test_Q_is_the_dense_marginal_log_likelihood_up_to_a_constant():
    rng, ubm, comp, x, post = _dense_model(11)
    C, D = ubm["means"].shape
    n, f, _, _ = R.stats64(x, post, [0, len(x)])
    ft = R.whiten(n, f, ubm)
    z = np.concatenate([(x[t] - ubm["means"][c]) / np.sqrt(ubm["variances"][c]) for t, c in enumerate(comp)])
    consts = []
    for k in range(4):
        T = np.zeros((C, R.padded(D), 2))
        T[:, :D] = rng.standard_normal((C, D, 2)) * (0.2 + k)
        S = np.eye(len(z)) + _dense_gaussian(ubm, comp, T) @ _dense_gaussian(ubm, comp, T).T
        ll = -0.5 * (np.linalg.slogdet(S)[1] + z @ np.linalg.solve(S, z))
        consts.append(ll - R.objective(n, ft, T))
    assert np.ptp(consts) < 1e-9 * max(1.0, abs(consts[0]))  # (-1/2 z.z: independent of T)


def test_Q_never_decreases_on_the_planted_set():
    for min_div in (False, True):
        _, Qs = IC.planted_em(min_div)
        assert len(Qs) == (7 if min_div else 4)
        assert (np.diff(Qs) >= 0).all(), Qs


# ------------------------------------------------------------------------------------- what the GPU tests rest on, on the oracle
def test_an_iteration_gains_100_times_the_change_from_the_statistics_bound():
    """3 iterations without minimum divergence: every iteration's gain of Q is at least 100 times what Q changes by when the
    statistics are replaced by values perturbed by their full bound (random signs), at each iteration's T."""
    p = IC.planted_stats()
    Ts, Qs = IC.planted_em(False)
    rng = np.random.default_rng(0)
    n2 = p["n"] + rng.choice([-1.0, 1.0], p["n"].shape) * p["dn"]
    f2 = p["f"] + rng.choice([-1.0, 1.0], p["f"].shape) * p["df"]
    ft2 = R.whiten(n2, f2, p["ubm"])
    gains = np.diff(Qs)
    for k, T in enumerate(Ts):
        change = abs(R.objective(n2, ft2, T) - R.objective(p["n"], p["ft"], T))
        print("iteration %d: gain %.6g, change %.6g" % (k + 1, gains[k], change))
        assert gains[k] >= 100.0 * change, (k, gains[k], change)


def test_the_oracle_ivectors_beat_the_utterance_means():
    p = IC.planted_stats()
    Ts, _ = IC.planted_em(True)
    w = R.estep(p["n"], p["ft"], Ts[-1])[0]
    U = len(p["labels"])
    means = np.stack([p["x"][int(a):int(b)].astype(np.float64).mean(axis=0) for a, b in zip(p["ptr"][:-1], p["ptr"][1:])])
    eer_iv, eer_mean = R.cosine_eer(w, p["labels"]), R.cosine_eer(means, p["labels"])
    print("cosine EER: i-vectors %.4f, utterance means %.4f (%d utterances)" % (eer_iv, eer_mean, U))
    assert eer_iv < eer_mean and eer_iv < 0.5


def test_the_sliced_statistics_stay_within_the_bound():
    x, post, ptr = IC.stats_inputs(4, (1025, 3, 0), 3, 5)
    n, f, an, af = R.stats64(x, post, ptr)
    dn, df = R.stats_bound(n, f, an, af)
    sn, sf = R.stats_sliced(x, post, ptr)
    assert (np.abs(sn - n) <= dn).all() and (np.abs(sf - f) <= df).all()
    assert not sn[2].any() and not sf[2].any()


# ------------------------------------------------------------------------------------------------------ the module's host side
def test_pack_and_unpack_round_trip():
    import ivector

    for R_ in (1, 2, 7, 128):
        i, j = ivector.tri_index(R_)
        assert np.array_equal(i * (i + 1) // 2 + j, np.arange(R_ * (R_ + 1) // 2)) and (j <= i).all()
        S = np.random.default_rng(R_).standard_normal((3, R_, R_))
        S = S + S.transpose(0, 2, 1)
        assert np.array_equal(ivector.unpack(ivector.pack(S), R_), S)
        St = torch.from_numpy(S)
        assert torch.equal(ivector.unpack(ivector.pack(St), R_), St)
    with pytest.raises(ValueError, match="no triangle"):
        ivector.unpack(np.zeros(5), 3)


def test_save_and_load_round_trip(tmp_path):
    import ivector

    rng = np.random.default_rng(2)
    model = {"T": rng.standard_normal((3 * 8, 4)), "means": rng.standard_normal((3, 5)), "variances": 1.0 + rng.random((3, 5))}
    path = str(tmp_path / "iv")  # (no ".npz" is added)
    ivector.save(path, model)
    back = ivector.load(path)
    assert sorted(back) == ["T", "means", "variances"] and all(back[k].dtype == np.float64 and np.array_equal(back[k], model[k]) for k in model)
    np.savez(str(tmp_path / "other.npz"), T=model["T"])
    with pytest.raises(ValueError, match="not a file ivector.save wrote"):
        ivector.load(str(tmp_path / "other.npz"))
    np.savez(str(tmp_path / "odd.npz"), T=model["T"][:-1], means=model["means"], variances=model["variances"])
    with pytest.raises(ValueError, match=r"are no \(C Dp, R\)"):
        ivector.load(str(tmp_path / "odd.npz"))


def test_chunks_hold_whole_utterances():
    import ivector

    ptr = np.array([0, 100, 100, 5000, 5010, 9000])
    for limit in (1, 200_000, 1 << 30):
        ch = ivector.utterance_chunks(ptr, 17, 39, limit)
        assert ch[0][0] == 0 and ch[-1][1] == 5 and all(a < b for a, b in ch) and all(x[1] == y[0] for x, y in zip(ch, ch[1:]))
    assert ivector.utterance_chunks(ptr, 17, 39, 1) == [(u, u + 1) for u in range(5)]  # (at least one utterance)
    assert ivector.utterance_chunks(ptr, 17, 39, 1 << 30) == [(0, 5)]
    assert len(ivector.utterance_chunks(ptr, 17, 39, 500_000)) > 1


def test_calls_refuse_cpu_tensors():
    import ivector

    with pytest.raises(RuntimeError, match="CPU tensor"):
        ivector.stats(torch.zeros(4, 8), torch.zeros(4, 3), torch.tensor([0, 4]))
    with pytest.raises(RuntimeError, match="device tensor"):
        ivector.solve(torch.ones(2, 3, dtype=torch.float64), torch.ones(2, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="device tensor"):
        ivector.whiten(torch.zeros(1, 3), torch.zeros(1, 3, 8), {"weights": np.ones(3), "means": np.zeros((3, 5)), "variances": np.ones((3, 5))})
    with pytest.raises(ValueError, match="rank"):
        ivector.fit(None, None, {"weights": np.ones(3), "means": np.zeros((3, 5)), "variances": np.ones((3, 5))}, 129)


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_signatures_match_the_header():
    import hip_binding as hb
    import ivector

    text = ext_abi.header_text("fhvae_ivector.h")
    found = ext_abi.declared("fhvae_ivector.h", "fhvae_iv_")
    assert found == ivector.IV_SIGNATURES
    assert sorted(found) == ["fhvae_iv_solve", "fhvae_iv_stats", "fhvae_iv_ws_bytes"]
    assert not set(found) & set(hb.SIGNATURES)
    for name, value in (("SLICE", ivector.IV_SLICE), ("MAX_RANK", ivector.IV_MAX_RANK), ("MAX_UTT", ivector.IV_MAX_UTT),
                        ("MAX_ROWS", ivector.IV_MAX_ROWS), ("MAX_COMP", ivector.IV_MAX_COMP)):
        assert int(re.search(r"#define FHVAE_IV_%s (\d+)" % name, text).group(1)) == value
    assert ivector.IV_SLICE == R.SLICE == 1024 and ivector.IV_MAX_RANK == 128
    for name, value in (("FHVAE_IV_BAD_PTR", ivector.IV_BAD_PTR), ("FHVAE_IV_NOT_PD", ivector.IV_NOT_PD)):
        assert int(re.search(r"%s = (\d+)" % name, text).group(1)) == value
    assert "no Kaldi binary" in open(os.path.join(ROOT, "include", "fhvae_ivector.h")).read()


def test_symbols_exported_and_the_main_header_untouched(lib):
    import hip_binding as hb
    import ivector

    for name in ivector.IV_SIGNATURES:
        assert hasattr(lib, name) and name not in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12 and len(hb.SIGNATURES) == 81  # include/fhvae_hip.h is untouched
    assert "fhvae_iv_" not in open(os.path.join(ROOT, "include", "fhvae_hip.h")).read().lower()


def test_workspace_matches_the_module_and_is_monotone(lib):
    import ivector

    f = lib.fhvae_iv_ws_bytes
    for Dp in (8, 40, 64):
        for C in (1, 65, 2048):
            last = 0
            for N, U in ((1, 1), (1024, 1), (1025, 1), (1025, 9), (360000, 360), (360000, 3600)):
                got = f(N, U, C, Dp)
                assert got == ivector.ws_bytes(N, U, C, Dp) and got > 0 and got >= last and got % 256 == 0, (N, U, C, Dp)
                last = got
    for bad in ((0, 1, 4, 8), (5, 0, 4, 8), (5, 1, 0, 8), (5, 1, 4, 0), (5, 1, 4, 12), (5, 1, 4, 72), ((1 << 30) + 1, 1, 4, 8),
                (5, (1 << 22) + 1, 4, 8), (5, 1, (1 << 20) + 1, 8)):
        assert f(*bad) == 0, bad


def test_stats_errors_before_any_launch(lib):
    keep, p = ext_abi.aligned()
    fn = lib.fhvae_iv_stats
    #       x ldx N   Dp post ldp C utt_ptr U ws ws_bytes n  f  status stream
    good = [p, 40, 100, 40, p, 20, 17, p, 3, p, 1 << 20, p, p, p, None]
    for i in (0, 4, 7, 9, 11, 12, 13):
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((2, 0), (2, -1), (8, 0), (8, -2), (6, 0), (3, 0), (3, 12), (3, 72), (3, 4), (1, 36), (5, 16), (10, 255), (10, 0)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i, bad in ((0, p + 4), (0, p + 8), (4, p + 4), (9, p + 8), (7, p + 4), (11, p + 2), (12, p + 1), (13, p + 2), (1, 42), (5, 18)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    assert fn(*_swap(good, 2, (1 << 30) + 1)) == LIMIT
    assert fn(*_swap(good, 8, (1 << 22) + 1)) == LIMIT
    assert fn(*_swap(_swap(good, 6, (1 << 20) + 1), 5, (1 << 20) + 4)) == LIMIT
    del keep


def test_solve_errors_before_any_launch(lib):
    keep, p = ext_abi.aligned()
    fn = lib.fhvae_iv_solve
    #       Lp b  U  R  w  E  logdet status stream
    good = [p, p, 5, 7, p, p, p, p, None]
    for i in (0, 1, 4, 7):
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((2, 0), (2, -1), (3, 0), (3, -5)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i in (0, 1, 4, 5, 6):
        assert fn(*_swap(good, i, p + 4)) == ALIGN, i
    assert fn(*_swap(good, 7, p + 2)) == ALIGN
    assert fn(*_swap(good, 3, 129)) == LIMIT and fn(*_swap(good, 2, (1 << 22) + 1)) == LIMIT
    del keep


# --------------------------------------------------------------------------------------------------------------------- CLI
def _stub_gpu(monkeypatch, corpora):
    """Everything that needs a device, replaced by the oracle: the archive's rows, the statistics, the fit and the extraction."""
    import extract_ivectors as EI
    import ivector

    calls = {"fit": 0}

    def corpus(args, feat_scp, len_scp):
        if feat_scp not in corpora:
            raise ValueError("%s: no such archive" % feat_scp)
        keys, x, ptr = corpora[feat_scp]
        return list(keys), torch.from_numpy(np.array(x)), ptr

    def utterance_stats(rows, ptr, ubm, max_bytes=0):
        x = rows.numpy()
        n, f, _, _ = R.stats64(x, R.posteriors(x, ubm).astype(np.float32), ptr)
        fp = np.zeros(f.shape[:2] + (R.padded(f.shape[2]),))
        fp[:, :, :f.shape[2]] = f
        return n, fp

    def fit(n, f, ubm, rank, iters=10, seed=0, min_div=True):
        calls["fit"] += 1
        C, D = ubm["means"].shape
        Ts, Qs = R.em(n, R.whiten(n, f[:, :, :D], ubm), R.start(C, D, rank, seed), iters, min_div)
        steps = ["init"] + (["m", "md"] * iters if min_div else ["m"] * iters)
        return {"T": Ts[-1].reshape(-1, rank), "means": ubm["means"], "variances": ubm["variances"]}, {"Q": Qs, "steps": steps}

    def extract(n, f, model, with_bad=False):
        C, D = model["means"].shape
        T = model["T"].reshape(C, R.padded(D), -1)
        w = R.estep(n, R.whiten(n, f[:, :, :D], model), T)[0]
        return (torch.from_numpy(w), 0) if with_bad else torch.from_numpy(w)

    monkeypatch.setattr(EI, "gpu_available", lambda: True)
    monkeypatch.setattr(EI, "corpus", corpus)
    monkeypatch.setattr(ivector, "utterance_stats", utterance_stats)
    monkeypatch.setattr(ivector, "fit", fit)
    monkeypatch.setattr(ivector, "extract", extract)
    return calls


def _small(tmp_path):
    import gmm

    p = IC.planted(seed=8, C=3, D=5, speakers=4, per_speaker=3, frames=30, rank=2)
    keys = ["s%02d-%d" % (s, u) for u, s in enumerate(p["labels"])]
    ubm = str(tmp_path / "ubm.npz")
    gmm.save(ubm, p["ubm"])
    return p, keys, ubm


def test_extract_ivectors_command_line(tmp_path, monkeypatch, capsys):
    import extract_ivectors as EI
    import ivector
    import score_speakers as SS

    p, keys, ubm = _small(tmp_path)
    calls = _stub_gpu(monkeypatch, {"eval.scp": (keys, p["x"], p["ptr"]), "train.scp": (keys[::-1], p["x"][::-1].copy(), p["ptr"])})
    out = tmp_path / "out"
    base = ["--feat-scp", "eval.scp", "--len-scp", "eval.len", "--ubm", ubm]
    assert EI.main(base + ["--rank", "2", "--iters", "2", "--seed", "5", "--out", str(out)]) == 0
    info = json.loads(capsys.readouterr().out)
    assert info == json.load(open(out / "ivector.json"))
    assert list(info) == ["rank", "C", "width", "utterances", "frames", "Q", "steps", "not_pd", "seed"]
    assert (info["rank"], info["C"], info["width"], info["utterances"], info["frames"], info["not_pd"], info["seed"]) == (2, 3, 5, 12, 360, 0, 5)
    assert len(info["Q"]) == 5 and info["steps"] == ["init", "m", "md", "m", "md"] and (np.diff(info["Q"]) >= 0).all()
    assert sorted(os.listdir(out)) == ["ivector.json", "ivector.npz", "ivectors.npy", "keys.txt", "ubm.npz"]
    w = np.load(out / "ivectors.npy")
    assert w.shape == (12, 2) and w.dtype == np.float64 and (out / "keys.txt").read_text().split() == keys
    # score_speakers.read_archive takes the directory as it is
    got_keys, rows = SS.read_archive(str(out))
    assert got_keys == keys and rows.dtype == np.float32 and np.array_equal(rows, w.astype(np.float32))
    # --model applies the saved extractor: no fit, the same bytes
    again = tmp_path / "again"
    assert EI.main(base + ["--model", str(out / "ivector.npz"), "--out", str(again)]) == 0
    capsys.readouterr()
    assert calls["fit"] == 1 and open(again / "ivectors.npy", "rb").read() == open(out / "ivectors.npy", "rb").read()
    assert json.load(open(again / "ivector.json"))["Q"] == []
    assert ivector.load(str(again / "ivector.npz"))["T"].shape == (3 * 8, 2)
    # a training archive of its own, --no-min-div, the Kaldi form
    third = tmp_path / "third"
    assert EI.main(base + ["--train-feat-scp", "train.scp", "--train-len-scp", "train.len", "--rank", "1", "--iters", "1", "--no-min-div",
                           "--out", str(third), "--out-format", "kaldi"]) == 0
    info3 = json.loads(capsys.readouterr().out)
    assert info3["steps"] == ["init", "m"] and info3["rank"] == 1 and os.path.exists(third / "feats.scp")
    k3, r3 = SS.read_archive(str(third))
    assert k3 == keys and r3.shape == (12, 1)


def test_extract_ivectors_errors(tmp_path, monkeypatch, capsys):
    import extract_ivectors as EI
    import ivector

    p, keys, ubm = _small(tmp_path)
    _stub_gpu(monkeypatch, {"eval.scp": (keys, p["x"], p["ptr"]), "wide.scp": (keys, np.zeros((360, 7), np.float32), p["ptr"])})
    base = ["--len-scp", "x.len", "--out", str(tmp_path / "o")]
    for argv in (["--feat-scp", "eval.scp", "--ubm", ubm, "--rank", "2", "--model", "m.npz"], ["--feat-scp", "eval.scp", "--ubm", ubm],
                 ["--feat-scp", "eval.scp", "--rank", "2"], ["--feat-scp", "eval.scp", "--ubm", ubm, "--rank", "129"],
                 ["--feat-scp", "eval.scp", "--ubm", ubm, "--rank", "2", "--train-feat-scp", "t.scp"]):
        with pytest.raises(SystemExit):
            EI.main(base + argv)
    capsys.readouterr()
    assert EI.main(base + ["--feat-scp", "missing.scp", "--ubm", ubm, "--rank", "2"]) == 1
    assert "missing.scp" in capsys.readouterr().err
    assert EI.main(base + ["--feat-scp", "wide.scp", "--ubm", ubm, "--rank", "2"]) == 1
    assert "wide.scp has 7 values per frame" in capsys.readouterr().err
    assert EI.main(base + ["--feat-scp", "eval.scp", "--ubm", str(tmp_path / "none.npz"), "--rank", "2"]) == 1
    assert "none.npz" in capsys.readouterr().err
    other = {"T": np.zeros((24, 2)), "means": p["ubm"]["means"] + 1.0, "variances": p["ubm"]["variances"]}
    ivector.save(str(tmp_path / "other.npz"), other)
    assert EI.main(base + ["--feat-scp", "eval.scp", "--ubm", ubm, "--model", str(tmp_path / "other.npz")]) == 1
    assert "other.npz was not fitted under this UBM" in capsys.readouterr().err
    monkeypatch.setattr(EI, "gpu_available", lambda: False)
    assert EI.main(base + ["--feat-scp", "eval.scp", "--ubm", ubm, "--rank", "2"]) == 1
    assert capsys.readouterr().err.strip() == "the mixture runs on a MI355X only (no CPU fallback)"


def test_read_archive_forms_and_messages(tmp_path):
    import score_speakers as SS

    rows = np.random.default_rng(0).standard_normal((4, 3))
    d = tmp_path / "iv"
    d.mkdir()
    np.save(d / "ivectors.npy", rows)
    (d / "keys.txt").write_text("a-1\na-2\nb-1\n")
    with pytest.raises(ValueError, match=r"ivectors.npy has shape \(4, 3\), keys.txt 3 keys"):
        SS.read_archive(str(d))
    (d / "keys.txt").write_text("a-1\na-2\nb-1\nb-1\n")
    with pytest.raises(ValueError, match="key 'b-1' is listed twice"):
        SS.read_archive(str(d))
    # mu2.npy still comes first, and the messages of the existing forms are what they were
    (d / "keys.txt").write_text("a-1\na-2\nb-1\nb-2\n")
    np.save(d / "mu2.npy", rows * 2)
    assert np.array_equal(SS.read_archive(str(d))[1], (rows * 2).astype(np.float32))
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match=r"empty: neither mu2.npy \+ keys.txt nor feats.scp"):
        SS.read_archive(str(empty))


def test_score_speakers_outputs_do_not_depend_on_the_archive_form(tmp_path, monkeypatch, capsys):
    """The same rows as mu2.npy + keys.txt (an existing input) and as ivectors.npy + keys.txt give the same bytes, and the existing
    form's report is the one verification.eer_from_hist gives: nothing about it changed."""
    import score_speakers as SS
    import spk_backend as SB
    import verification as V

    def speaker_verification(emb, labels, n_bins=4096, device=None):
        e = np.asarray(emb, dtype=np.float64)
        e = e / np.linalg.norm(e, axis=1, keepdims=True)
        i, j = np.triu_indices(len(e), 1)
        s = (e[i] * e[j]).sum(axis=1)
        b = np.clip(np.floor((s + 1.0) / 2.0 * n_bins), 0, n_bins - 1).astype(np.int64)
        hist = np.zeros((2, n_bins), dtype=np.int64)
        same = np.asarray(labels)[i] == np.asarray(labels)[j]
        np.add.at(hist[0], b[same], 1)
        np.add.at(hist[1], b[~same], 1)
        return dict(V.eer_from_hist(hist), hist=hist)

    monkeypatch.setattr(V, "speaker_verification", speaker_verification)
    rng = np.random.default_rng(3)
    spk = np.repeat(np.arange(5), 4)
    rows = (rng.standard_normal((5, 6))[spk] + 0.5 * rng.standard_normal((20, 6))).astype(np.float32)
    keys = ["s%d-%d" % (s, u) for u, s in enumerate(spk)]
    outs = []
    for name in ("mu2.npy", "ivectors.npy"):
        d = tmp_path / name.split(".")[0]
        d.mkdir()
        np.save(d / name, rows)
        (d / "keys.txt").write_text("".join(k + "\n" for k in keys))
        out = tmp_path / ("out_" + name.split(".")[0])
        assert SS.main(["--eval-emb", str(d), "--spk-key-sep", "-", "--bins", "64", "--out", str(out)]) == 0
        capsys.readouterr()
        outs.append({f: open(out / f, "rb").read() for f in sorted(os.listdir(out))})
    assert outs[0] == outs[1] and sorted(outs[0]) == ["hist_cosine.npy", "speakers.json"]
    report = json.loads(outs[0]["speakers.json"])
    want = speaker_verification(rows, V.labels_from_speakers([k.split("-")[0] for k in keys])[0], 64)
    hist = want.pop("hist")
    assert report["cosine"] == json.loads(json.dumps(dict(SB.eer_from_hist(hist, -1.0, 1.0))))
    assert list(report) == ["sequences", "speakers", "unlabelled", "bins", "cosine"]
