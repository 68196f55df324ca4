"""i-vector extraction on the GPU: fhvae_iv_stats and fhvae_iv_solve against the float64 oracle (tests/ivector_ref.py) on the shared
cases (tests/ivector_cases.py), their failure handling and determinism, and extract / fit end to end on the planted set.  The two
conditions the end-to-end tests rest on are proved on the oracle alone in tests/test_ivector_cpu.py."""
import numpy as np
import pytest
import torch

import ivector_cases as IC
import ivector_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def iv():
    import build_ext

    build_ext.build(verbose=False)
    import ivector

    assert torch.cuda.is_available()
    return ivector


def dev(t):
    return torch.from_numpy(np.array(t)).cuda()  # (a copy: read-only arrays)


def bits(t):
    a = np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def gpu_stats(iv, x, post, ptr, extra=0):
    """stats() on device copies; `extra` widens the leading dimensions of x and post beyond their widths."""
    D, C = x.shape[1], post.shape[1]
    Dp = R.padded(D)
    xd = torch.zeros(x.shape[0], Dp + extra, device="cuda")
    xd[:, :D] = dev(x)
    pd = torch.zeros(post.shape[0], (C + 3) // 4 * 4 + extra, device="cuda")
    pd[:, :C] = dev(post)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    n, f = iv.stats(xd[:, :Dp], pd[:, :C], dev(ptr), status=status)
    assert n.dtype == torch.float32 and f.dtype == torch.float32 and tuple(n.shape) == (len(ptr) - 1, C) and tuple(f.shape) == (len(ptr) - 1, C, Dp)
    return n.cpu().numpy(), f.cpu().numpy(), int(status.item())


# -------------------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("name", sorted(IC.STATS_CASES))
def test_stats_within_the_bound_of_the_float64_sums(iv, name):
    lengths, C, D, extra = IC.STATS_CASES[name]
    x, post, ptr = IC.stats_inputs(sorted(IC.STATS_CASES).index(name), lengths, C, D)
    n, f, st = gpu_stats(iv, x, post, ptr, extra)
    assert st == 0
    wn, wf, an, af = R.stats64(x, post, ptr)
    dn, df = R.stats_bound(wn, wf, an, af)
    share = max(float((np.abs(n - wn) / np.maximum(dn, 1e-300)).max()), float((np.abs(f[:, :, :D] - wf) / np.maximum(df, 1e-300)).max()))
    print("%s: the worst entry uses %.4f of its bound" % (name, share))
    assert (np.abs(n - wn) <= dn).all() and (np.abs(f[:, :, :D] - wf) <= df).all()
    assert not f[:, :, D:].any()  # the padding columns
    for u, length in enumerate(lengths):
        if length == 0:
            assert not n[u].any() and not f[u].any()


def test_stats_of_short_one_hot_utterances_are_exact(iv):
    """At most 4 rows enter one MFMA; with one-hot posteriors and values that are multiples of 1/16 below 8 every product and every
    sum is exact in f32 in any order, so the result equals the float64 sums."""
    rng = np.random.default_rng(5)
    lengths = (0, 1, 2, 3, 4, 4, 3, 2, 1)
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    N, C, D = int(ptr[-1]), 5, 13
    x = (rng.integers(-127, 128, (N, D)) / 16.0).astype(np.float32)
    post = np.eye(C, dtype=np.float32)[rng.integers(0, C, N)]
    n, f, st = gpu_stats(iv, x, post, ptr)
    wn, wf, _, _ = R.stats64(x, post, ptr)
    assert st == 0 and np.array_equal(n.astype(np.float64), wn) and np.array_equal(f[:, :, :D].astype(np.float64), wf)


def test_stats_are_bitwise_the_same_alone_in_a_batch_and_permuted(iv):
    C, D = 17, 39
    x, post, ptr = IC.stats_inputs(77, IC.LENGTHS, C, D)
    n, f, st = gpu_stats(iv, x, post, ptr)
    assert st == 0
    perm = [4, 8, 0, 6, 2, 7, 1, 5, 3]
    xs, ps = [x[int(ptr[u]):int(ptr[u + 1])] for u in range(9)], [post[int(ptr[u]):int(ptr[u + 1])] for u in range(9)]
    pptr = np.concatenate([[0], np.cumsum([IC.LENGTHS[u] for u in perm])]).astype(np.int64)
    n2, f2, _ = gpu_stats(iv, np.concatenate([xs[u] for u in perm]), np.concatenate([ps[u] for u in perm]), pptr)
    for k, u in enumerate(perm):
        assert np.array_equal(bits(n2[k]), bits(n[u])) and np.array_equal(bits(f2[k]), bits(f[u])), u
    for u in range(9):
        if IC.LENGTHS[u] == 0:
            n1, f1, _ = gpu_stats(iv, x[:1], post[:1], np.array([0, 0], dtype=np.int64))  # (an empty utterance alone, one unused row)
        else:
            n1, f1, _ = gpu_stats(iv, xs[u], ps[u], np.array([0, IC.LENGTHS[u]], dtype=np.int64))
        assert np.array_equal(bits(n1[0]), bits(n[u])) and np.array_equal(bits(f1[0]), bits(f[u])), u


@pytest.mark.parametrize("ptr", [(0, 10, 5, 30, 40), (0, 10, 50, 30, 40), (-1, 10, 20, 1100, 40), (0, 10, 20, 41, 40)])
def test_a_bad_pointer_zeroes_its_utterance_and_no_other(iv, ptr):
    x, post, _ = IC.stats_inputs(9, (40,), 6, 5)
    ptr = np.array(ptr, dtype=np.int64)
    n, f, st = gpu_stats(iv, x, post, ptr)
    assert st == iv.IV_BAD_PTR
    good = [0 <= ptr[u] <= ptr[u + 1] <= 40 for u in range(4)]
    assert not all(good) and any(good)
    for u in range(4):
        if good[u]:
            a, b = int(ptr[u]), int(ptr[u + 1])
            n1, f1, st1 = gpu_stats(iv, x[a:b], post[a:b], np.array([0, b - a], dtype=np.int64))
            assert st1 == 0 and np.array_equal(bits(n[u]), bits(n1[0])) and np.array_equal(bits(f[u]), bits(f1[0])), u
        else:
            assert not n[u].any() and not f[u].any(), u


def test_utterance_stats_do_not_depend_on_the_chunks(iv):
    """utterance_stats (gmm.loglik / posteriors, then stats) in one chunk and in chunks of one utterance: the same bits, and the
    statistics of gmm.posteriors' own posteriors."""
    import gmm

    p = IC.planted(seed=8, C=5, D=13, speakers=3, per_speaker=3, frames=300, rank=2)
    lengths = [300, 0, 1100, 300, 1, 399, 300, 200, 100]
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    rows = dev(p["x"])
    n, f = iv.utterance_stats(rows, ptr, p["ubm"])
    n1, f1 = iv.utterance_stats(rows, ptr, p["ubm"], max_bytes=1)
    assert np.array_equal(bits(n), bits(n1)) and np.array_equal(bits(f), bits(f1))
    tab, cst = gmm.table({k: torch.from_numpy(v) for k, v in p["ubm"].items()}, rows.device)
    xp = torch.nn.functional.pad(rows, (0, 3))
    post = gmm.posteriors(xp, tab, cst, gmm.loglik(xp, tab, cst)[0])
    wn, wf, an, af = R.stats64(p["x"], post.cpu().numpy(), ptr)
    dn, df = R.stats_bound(wn, wf, an, af)
    assert (np.abs(n.cpu().numpy() - wn) <= dn).all() and (np.abs(f.cpu().numpy()[:, :, :13] - wf) <= df).all()
    assert abs(float(n.sum()) - 2700.0) < 0.01 and not f[1].any()


# ------------------------------------------------------------------------------------------------------------------- solve
def gpu_solve(iv, L, b, want_E=True, want_logdet=True):
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    w, E, ld = iv.solve(dev(iv.pack(L)), dev(b), want_E=want_E, want_logdet=want_logdet, status=status)
    return (w.cpu().numpy(), None if E is None else E.cpu().numpy(), None if ld is None else ld.cpu().numpy(), int(status.item()))


@pytest.mark.parametrize("R_,U", IC.SOLVE_CASES)
def test_solve_within_the_cholesky_forward_bound(iv, R_, U):
    """w, E and logdet within R^2 2^-52 kappa_2(L_u): w and E in the 2-norm relative to the oracle's, logdet relative to R."""
    L, b = IC.solve_inputs(1000 + R_, R_, U)
    w, E, ld, st = gpu_solve(iv, L, b)
    assert st == 0 and w.shape == (U, R_) and E.shape == (U, R_ * (R_ + 1) // 2) and ld.shape == (U,)
    Ef = iv.unpack(E, R_)
    worst = 0.0
    for u in range(U):
        ev = np.linalg.eigvalsh(L[u])
        kappa = ev[-1] / ev[0]
        assert ev[0] > 0 and kappa <= 1e6
        bound = R_ * R_ * R.U52 * kappa
        ww, wE, wld = R.solve(L[u], b[u])
        errs = (np.linalg.norm(w[u] - ww) / np.linalg.norm(ww), np.linalg.norm(Ef[u] - wE, 2) / np.linalg.norm(wE, 2), abs(ld[u] - wld) / R_)
        worst = max(worst, max(errs) / bound)
        assert max(errs) <= bound, (u, errs, bound)
    print("R = %d, U = %d: the worst result uses %.4f of its bound" % (R_, U, worst))


@pytest.mark.parametrize("R_", [1, 9, 33, 100])
def test_a_matrix_that_is_not_positive_definite_fails_alone(iv, R_):
    L, b = IC.solve_inputs(50 + R_, R_, 7)
    w, E, ld, st = gpu_solve(iv, L, b)
    bad = L.copy()
    v = np.linalg.eigh(bad[3])[1][:, R_ // 2]
    bad[3] = bad[3] - (np.linalg.eigvalsh(bad[3])[R_ // 2] + 1.0) * np.outer(v, v)  # (one eigenvalue becomes -1)
    assert np.linalg.eigvalsh(bad[3]).min() < -0.5
    w2, E2, ld2, st2 = gpu_solve(iv, bad, b)
    assert st == 0 and st2 == iv.IV_NOT_PD
    assert np.isnan(w2[3]).all() and np.isnan(E2[3]).all() and np.isnan(ld2[3])
    keep = [u for u in range(7) if u != 3]
    for got, want in ((w2, w), (E2, E), (ld2, ld)):
        assert np.array_equal(bits(got[keep]), bits(want[keep])) and not np.isnan(got[keep]).any()


@pytest.mark.parametrize("R_", [7, 32, 33, 64, 128])
def test_solve_is_bitwise_the_same_alone_and_in_a_batch(iv, R_):
    L, b = IC.solve_inputs(200 + R_, R_, 11)
    w, E, ld, _ = gpu_solve(iv, L, b)
    for u in (0, 5, 10):
        w1, E1, ld1, _ = gpu_solve(iv, L[u:u + 1], b[u:u + 1])
        assert np.array_equal(bits(w1[0]), bits(w[u])) and np.array_equal(bits(E1[0]), bits(E[u])) and np.array_equal(bits(ld1), bits(ld[u:u + 1]))
    w3, E3, ld3, _ = gpu_solve(iv, L[::-1], b[::-1], want_E=False, want_logdet=False)
    assert E3 is None and ld3 is None and np.array_equal(bits(w3[::-1]), bits(w))  # (w does not depend on what else is asked for)


# --------------------------------------------------------------------------------------------------------------- end to end
def _device_stats(iv):
    p = IC.planted_stats()
    n, f = iv.stats(dev(np.pad(p["x"], ((0, 0), (0, 3)))), dev(p["post"]), dev(p["ptr"]))
    return p, n, f


def test_extract_reproduces_the_oracle_ivectors(iv):
    """The device's statistics of the same f32 post, then extract with the oracle's model, against the oracle's i-vectors from its
    float64 statistics.  With dn, df the statistics' bounds, dft_c = (df_c + dn_c |m_c|) / s_c (plus 4 roundings of the float64
    whitening), and the float64 rounding of the two dense products:
        |db| <= |Tt|^T dft + (C Dp + 2) 2^-53 |Tt|^T |ft|          ||dL||_2 <= sum_c (dn_c + (C + 2) 2^-53 n_c) ||M_c||_2
        ||dw|| <= ||L^-1|| (||db|| + ||dL|| ||w||) / (1 - ||L^-1|| ||dL||)  +  R^2 2^-52 kappa_2(L) ||w||
    the first term the statistics' bound carried through Tt^T and L^-1 (the exact perturbation bound of a linear system), the
    second the solve's."""
    p, n, f = _device_stats(iv)
    Ts, _ = IC.planted_em(True)
    T = Ts[-1]
    C, Dp, R_ = T.shape
    D = p["ubm"]["means"].shape[1]
    model = {"T": T.reshape(C * Dp, R_), "means": p["ubm"]["means"], "variances": p["ubm"]["variances"]}
    w = iv.extract(n, f, model).cpu().numpy()
    want = R.estep(p["n"], p["ft"], T)[0]
    s = np.sqrt(p["ubm"]["variances"])
    dft = np.zeros_like(p["ft"])
    dft[:, :, :D] = (p["df"] + p["dn"][:, :, None] * np.abs(p["ubm"]["means"])[None]) / s[None]
    dft[:, :, :D] += 4 * 2.0 ** -53 * (np.abs(p["f"]) + p["n"][:, :, None] * np.abs(p["ubm"]["means"])[None]) / s[None]  # (whitening in float64)
    absT = np.abs(T).reshape(C * Dp, R_)
    U = want.shape[0]
    db = dft.reshape(U, -1) @ absT + (C * Dp + 2) * 2.0 ** -53 * (np.abs(p["ft"]).reshape(U, -1) @ absT)
    m2 = np.array([np.linalg.norm(T[c].T @ T[c], 2) for c in range(C)])
    dL = (p["dn"] + (C + 2) * 2.0 ** -53 * p["n"]) @ m2
    worst = 0.0
    for u in range(U):
        ev = np.linalg.eigvalsh(R.precision(p["n"][u], T))
        li, nw = 1.0 / ev[0], np.linalg.norm(want[u])
        bound = li * (np.linalg.norm(db[u]) + dL[u] * nw) / (1.0 - li * dL[u]) + R_ * R_ * R.U52 * (ev[-1] / ev[0]) * nw
        err = np.linalg.norm(w[u] - want[u])
        worst = max(worst, err / bound)
        assert err <= bound, (u, err, bound)
    print("extract: the worst utterance uses %.4f of its bound" % worst)


def test_fit_is_never_an_iteration_behind_the_oracle(iv):
    """3 iterations without minimum divergence (the setting tests/test_ivector_cpu.py proves the margin for): the oracle's Q of the
    device-fitted T after iteration k is at least the oracle's own Q after iteration k - 1, and the device's own Q is monotone.
    Then with minimum divergence: monotone over every step, and the device i-vectors' cosine EER below the utterance means'."""
    p, n, f = _device_stats(iv)
    _, Qs = IC.planted_em(False)
    C, D = p["ubm"]["means"].shape
    for k in (1, 2, 3):
        model, hist = iv.fit(n, f, p["ubm"], 3, iters=k, seed=0, min_div=False)
        assert hist["steps"] == ["init"] + ["m"] * k and (np.diff(hist["Q"]) >= 0).all(), hist
        q = R.objective(p["n"], p["ft"], model["T"].reshape(C, R.padded(D), 3))
        print("iteration %d: the oracle's Q of the device's T %.6f, the oracle's own %.6f, before it %.6f" % (k, q, Qs[k], Qs[k - 1]))
        assert q >= Qs[k - 1]
    model, hist = iv.fit(n, f, p["ubm"], 3, iters=3, seed=0)
    assert hist["steps"] == ["init", "m", "md", "m", "md", "m", "md"] and (np.diff(hist["Q"]) >= 0).all(), hist
    w = iv.extract(n, f, model).cpu().numpy()
    means = np.stack([p["x"][int(a):int(b)].astype(np.float64).mean(axis=0) for a, b in zip(p["ptr"][:-1], p["ptr"][1:])])
    eer_iv, eer_mean = R.cosine_eer(w, p["labels"]), R.cosine_eer(means, p["labels"])
    print("cosine EER: device i-vectors %.4f, utterance means %.4f" % (eer_iv, eer_mean))
    assert eer_iv < eer_mean


def test_a_saved_model_reproduces_the_ivectors_byte_for_byte(iv, tmp_path):
    p, n, f = _device_stats(iv)
    model, _ = iv.fit(n, f, p["ubm"], 3, iters=1, seed=1)
    iv.save(str(tmp_path / "m.npz"), model)
    a, b = iv.extract(n, f, model), iv.extract(n, f, iv.load(str(tmp_path / "m.npz")))
    assert np.array_equal(bits(a), bits(b)) and a.dtype == torch.float64 and tuple(a.shape) == (240, 3)


def test_extract_ivectors_command_line_end_to_end(iv, tmp_path, capsys):
    """The planted set as a numpy archive through extract_ivectors.py: a UBM fitted here, the extractor, the archive
    score_speakers.py reads; --model with the files of the first run gives the same bytes."""
    import json

    import extract_ivectors as EI
    import score_speakers as SS

    p = IC.planted(seed=4, speakers=8, per_speaker=6, frames=150)
    keys = ["s%02d-%02d" % (s, u) for u, s in enumerate(p["labels"])]
    with open(tmp_path / "feats.scp", "w") as fs, open(tmp_path / "len.scp", "w") as ls:
        for u, key in enumerate(keys):
            np.save(tmp_path / (key + ".npy"), p["x"][int(p["ptr"][u]):int(p["ptr"][u + 1])])
            fs.write("%s %s\n" % (key, tmp_path / (key + ".npy")))
            ls.write("%s %d\n" % (key, 150))
    base = ["--feat-scp", str(tmp_path / "feats.scp"), "--len-scp", str(tmp_path / "len.scp")]
    out = tmp_path / "out"
    assert EI.main(base + ["--ubm-k", "6", "--ubm-iters", "5", "--rank", "3", "--iters", "2", "--out", str(out)]) == 0
    info = json.loads(capsys.readouterr().out.strip().splitlines()[-1])  # (the dataset prints a line of its own before it)
    assert info == json.load(open(out / "ivector.json"))
    assert (info["rank"], info["C"], info["width"], info["utterances"], info["frames"], info["not_pd"]) == (3, 6, 5, 48, 7200, 0)
    assert len(info["Q"]) == 5 and (np.diff(info["Q"]) >= 0).all()
    got_keys, rows = SS.read_archive(str(out))
    assert got_keys == keys and rows.shape == (48, 3) and np.isfinite(rows).all()
    means = np.stack([p["x"][int(a):int(b)].astype(np.float64).mean(axis=0) for a, b in zip(p["ptr"][:-1], p["ptr"][1:])])
    assert R.cosine_eer(rows, p["labels"]) < R.cosine_eer(means, p["labels"])
    again = tmp_path / "again"
    assert EI.main(base + ["--ubm", str(out / "ubm.npz"), "--model", str(out / "ivector.npz"), "--out", str(again)]) == 0
    capsys.readouterr()
    assert open(again / "ivectors.npy", "rb").read() == open(out / "ivectors.npy", "rb").read()
