"""The mixture without a GPU: the oracle (tests/gmm_ref.py) against itself, gmm.mstep against the oracle's, save / load, the
chunking of estep, GMM_SIGNATURES against include/fhvae_gmm.h, the entry points' argument errors (they return before any
launch), the workspace size, the refusals of the raw calls and fit_gmm.py's argument errors."""
import os
import re

import numpy as np
import pytest
import torch

import gmm_ref as R
import ext_abi
from ext_abi import aligned as _aligned, swap as _swap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, ALIGN, LIMIT = -1, -2, -4, -5


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import gmm

    return gmm.load_library()


def blobs(n=300, K=4, D=5, seed=3):
    rng = np.random.default_rng(seed)
    centres = 6.0 * rng.standard_normal((K, D))
    x = np.concatenate([centres[k] + rng.standard_normal((n, D)) for k in range(K)]).astype(np.float32)
    return x, centres


# ------------------------------------------------------------------------------------------------------------------ oracle
def test_oracle_against_itself():
    x, w, mu, var = R.case(200, 7, 13)
    w[3] = 0.0
    w /= w.sum()
    tab, cst = R.table(w, mu, var)
    assert tab.shape == (7, 32) and tab.dtype == np.float32 and cst[3] == -np.inf and not tab[:, 13:16].any() and not tab[:, 29:].any()
    e = R.estep(x, tab, cst)
    assert np.allclose(e["post"].sum(axis=1), 1.0, rtol=0, atol=1e-13) and not e["post"][:, 3].any() and not (e["labels"] == 3).any()
    # against the density itself: the f32 rounding of the table is what separates them, so from a float64 "table" here
    tab64 = np.zeros((7, 32))
    tab64[:, :13], tab64[:, 16:29] = mu / var, -0.5 / var
    with np.errstate(divide="ignore"):
        cst64 = np.log(w) - 0.5 * (13 * np.log(2 * np.pi) + np.log(var).sum(axis=1) + (mu * mu / var).sum(axis=1))
    feat = np.concatenate([R.pad_rows(x).astype(np.float64), R.pad_rows(x).astype(np.float64) ** 2], axis=1)
    l = feat @ tab64.T + cst64
    m = l.max(axis=1)
    ll = m + np.log(np.exp(l - m[:, None]).sum(axis=1))
    assert np.allclose(ll, R.direct_loglik(x, w, mu, var), rtol=1e-12, atol=0)
    l32, M = R.scores(x, tab, cst)
    finite = np.isfinite(l32)
    assert np.all(M[finite] >= np.abs(l32[finite])) and np.all(e["gap"] >= 0) and np.all(e["E"] >= 0) and np.all(e["Emax"] > 0)
    one = R.estep(x, *R.table(w[:1] / w[0], mu[:1], var[:1]))
    assert np.all(one["gap"] == np.inf) and np.allclose(one["post"], 1.0)


def test_oracle_em_step_does_not_lower_the_likelihood():
    x, centres = blobs()
    K, D = centres.shape
    gvar = x.astype(np.float64).var(axis=0)
    rng = np.random.default_rng(0)
    model = (np.full(K, 1.0 / K), centres + rng.standard_normal((K, D)), np.tile(gvar, (K, 1)))
    last = None
    for _ in range(6):
        ll, model = R.em_step(x, *model, gvar)
        assert last is None or ll >= last - 1e-9
        last = ll
    assert np.allclose(model[0], 0.25, atol=0.02)


# ------------------------------------------------------------------------------------------------------------------- mstep
def test_mstep_equals_the_oracle():
    import gmm

    rng = np.random.default_rng(5)
    K, D, n = 6, 5, 1000
    nk = rng.uniform(50, 300, K)
    mu_t = rng.standard_normal((K, D))
    var_t = np.exp(rng.uniform(-1, 1, (K, D)))
    nk[2] = 2.5          # starved: below min_count
    nk[4] = 0.0          # starved: no mass at all
    var_t[1, 3] = 1e-6   # floored
    var_t[5, 0] = 1e-9   # floored
    sx, sxx = nk[:, None] * mu_t, nk[:, None] * (var_t + mu_t * mu_t)
    prev_mu, prev_var = rng.standard_normal((K, D)), np.exp(rng.uniform(-1, 1, (K, D)))
    gvar = np.exp(rng.uniform(-0.5, 0.5, D))
    want = R.mstep(nk, sx, sxx, prev_mu, prev_var, n, gvar)
    assert want[3] == 2 and want[4] == 2
    stats = {"nk": torch.from_numpy(nk), "sx": torch.from_numpy(sx), "sxx": torch.from_numpy(sxx)}
    model, starved, floored = gmm.mstep(stats, {"means": prev_mu, "variances": prev_var}, n, gvar)
    assert (starved, floored) == (2, 2)
    for got, ref in zip((model["weights"], model["means"], model["variances"]), want[:3]):
        assert got.dtype == torch.float64 and np.allclose(got.numpy(), ref, rtol=1e-12, atol=0)
    assert np.array_equal(model["means"].numpy()[[2, 4]], prev_mu[[2, 4]]) and np.array_equal(model["variances"].numpy()[[2, 4]], prev_var[[2, 4]])
    assert model["variances"].numpy()[1, 3] == 0.01 * gvar[3] and model["variances"].numpy()[5, 0] == 0.01 * gvar[0]
    loose = gmm.mstep(stats, {"means": prev_mu, "variances": prev_var}, n, gvar, var_floor=1e-12, min_count=1.0)
    want = R.mstep(nk, sx, sxx, prev_mu, prev_var, n, gvar, var_floor=1e-12, min_count=1.0)
    assert (loose[1], loose[2]) == (1, 0) == want[3:] and np.allclose(loose[0]["variances"].numpy(), want[2], rtol=1e-12, atol=0)


def test_save_load_round_trip(tmp_path):
    import gmm

    rng = np.random.default_rng(9)
    model = {"weights": rng.dirichlet(np.ones(5)), "means": rng.standard_normal((5, 13)), "variances": np.exp(rng.standard_normal((5, 13)))}
    path = str(tmp_path / "gmm.npz")
    gmm.save(path, {k: torch.from_numpy(v) for k, v in model.items()})
    back = gmm.load(path)
    assert sorted(back) == ["means", "variances", "weights"] and sorted(os.listdir(tmp_path)) == ["gmm.npz"]
    for k in model:
        assert back[k].dtype == np.float64 and np.array_equal(back[k].view(np.int64), model[k].view(np.int64))
    np.savez(str(tmp_path / "bad.npz"), weights=model["weights"])
    with pytest.raises(ValueError, match="means"):
        gmm.load(str(tmp_path / "bad.npz"))
    np.savez(str(tmp_path / "odd.npz"), weights=model["weights"], means=model["means"], variances=model["variances"][:4])
    with pytest.raises(ValueError):
        gmm.load(str(tmp_path / "odd.npz"))


# ---------------------------------------------------------------------------------------------------------------- chunking
@pytest.mark.parametrize("K", [1, 130, 1000])
def test_chunks_are_slices_that_cover_the_rows_within_the_budget(lib, K):
    import gmm

    S = gmm.GMM_SLICE
    ldp = (K + 3) // 4 * 4
    for width in (32, 39):
        Dp = gmm.padded(width)
        one = S * ldp * 4 + int(lib.fhvae_gmm_ws_bytes(S, K, Dp))
        for max_bytes in (one, 3 * one + 17, 512 << 20):
            for N in (1, S - 1, S, S + 1, 3 * S, 3 * S + 5, 10 * S - 1):
                chunks = gmm.chunk_rows(N, K, width, max_bytes)
                assert sum(chunks) == N and all(c > 0 for c in chunks)
                assert all(c % S == 0 for c in chunks[:-1]) and len(set(chunks[:-1])) <= 1 and chunks[-1] <= chunks[0]
                for c in chunks:
                    ws = int(lib.fhvae_gmm_ws_bytes(c, K, Dp))
                    assert ws == gmm.ws_bytes(c, K, Dp) and c * ldp * 4 + ws <= max_bytes, (N, K, width, max_bytes, c)
                assert chunks == gmm.chunk_rows(N, K, width, max_bytes)
            if max_bytes == one:
                assert gmm.chunk_rows(3 * S + 5, K, width, max_bytes) == [S, S, S, 5]
        with pytest.raises(ValueError, match="no slice"):
            gmm.chunk_rows(5000, K, width, one - 1)


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_signatures_match_the_header():
    import gmm
    import hip_binding as hb

    text = ext_abi.header_text("fhvae_gmm.h")
    found = ext_abi.declared("fhvae_gmm.h", "fhvae_gmm_")
    assert found == gmm.GMM_SIGNATURES
    assert sorted(found) == ["fhvae_gmm_loglik", "fhvae_gmm_post", "fhvae_gmm_stats", "fhvae_gmm_ws_bytes"]
    assert not set(found) & set(hb.SIGNATURES)
    for name, value in (("SLICE", gmm.GMM_SLICE), ("MAX_DP", gmm.GMM_MAX_DP), ("MAX_ROWS", gmm.GMM_MAX_ROWS), ("MAX_COMP", gmm.GMM_MAX_COMP)):
        assert int(re.search(r"#define FHVAE_GMM_%s (\d+)" % name, text).group(1)) == value
    assert gmm.GMM_SLICE == R.SLICE == 1024 and gmm.GMM_MAX_ROWS == 2 ** 30 and gmm.GMM_MAX_COMP == 2 ** 20 and gmm.GMM_MAX_DP == 64


def test_symbols_exported_and_the_main_header_untouched(lib):
    import gmm
    import hip_binding as hb

    for name in gmm.GMM_SIGNATURES:
        assert hasattr(lib, name) and name not in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12 and len(hb.SIGNATURES) == 81  # include/fhvae_hip.h is untouched
    header = open(os.path.join(ROOT, "include", "fhvae_hip.h")).read()
    assert "fhvae_gmm_" not in header and "gmm" not in header.lower()


def test_loglik_errors_before_any_launch(lib):
    keep, p = _aligned()
    fn = lib.fhvae_gmm_loglik
    #       x ldx N  Dp tab ldt cst K loglik label stream
    good = [p, 32, 4, 32, p, 64, p, 2, p, p, None]
    for i in (0, 4, 6, 8):
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((3, 0), (3, 4), (3, 12), (3, 72), (3, -8), (1, 24), (5, 48), (5, 63), (2, 0), (2, -1), (7, 0), (7, -3)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i, bad in ((0, p + 4), (4, p + 8), (1, 34), (5, 66), (6, p + 2), (8, p + 1), (9, p + 2)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    assert fn(*_swap(good, 2, (1 << 30) + 1)) == LIMIT and fn(*_swap(good, 7, (1 << 20) + 1)) == LIMIT
    # every width of the rule passes the shape checks (a misaligned pointer stops the call before a launch)
    for Dp in range(8, 72, 8):
        assert fn(p + 4, Dp, 4, Dp, p, 2 * Dp, p, 2, p, p, None) == ALIGN, Dp
    del keep


def test_post_errors_before_any_launch(lib):
    keep, p = _aligned()
    fn = lib.fhvae_gmm_post
    #       x ldx N  Dp tab ldt cst K loglik post ldp stream
    good = [p, 32, 4, 32, p, 64, p, 6, p, p, 8, None]
    for i in (0, 4, 6, 8, 9):
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((3, 12), (3, 72), (1, 24), (5, 56), (2, 0), (7, 0), (10, 4), (10, 5)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i, bad in ((0, p + 4), (4, p + 8), (1, 33), (5, 65), (6, p + 2), (8, p + 2), (9, p + 4), (10, 10), (10, 7)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    assert fn(*_swap(good, 2, (1 << 30) + 1)) == LIMIT
    big = _swap(_swap(good, 7, (1 << 20) + 1), 10, (1 << 20) + 4)
    assert fn(*big) == LIMIT
    del keep


def test_stats_errors_before_any_launch(lib):
    keep, p = _aligned()
    ws = lib.fhvae_gmm_ws_bytes(4, 6, 32)
    fn = lib.fhvae_gmm_stats
    #       x ldx N  Dp post ldp K ws ws_bytes nk sx sxx accumulate stream
    good = [p, 32, 4, 32, p, 8, 6, p, ws, p, p, p, 0, None]
    for i in (0, 4, 7, 9, 10, 11):
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((3, 12), (3, 72), (3, 0), (1, 24), (2, 0), (6, 0), (5, 4), (8, ws - 1), (8, 0)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i, bad in ((0, p + 4), (4, p + 8), (1, 34), (5, 10), (7, p + 8), (9, p + 4), (10, p + 4), (11, p + 2)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    assert fn(*_swap(good, 2, (1 << 30) + 1)) == LIMIT
    assert fn(*_swap(_swap(good, 6, (1 << 20) + 1), 5, (1 << 20) + 4)) == LIMIT
    del keep


def test_workspace_is_positive_and_monotone(lib):
    f = lib.fhvae_gmm_ws_bytes
    for Dp in (8, 16, 40, 64):
        last = 0
        for N in (1, 2, 1023, 1024, 1025, 2500, 359280, 3592800, 1 << 30):
            v = f(N, 100, Dp)
            assert v > 0 and v >= last and v % 256 == 0, (N, Dp)
            last = v
        last = 0
        for K in (1, 2, 63, 64, 65, 1000, 1 << 20):
            v = f(100000, K, Dp)
            assert v > 0 and v >= last, (K, Dp)
            last = v
    assert f(1024, 10, 32) < f(1025, 10, 32) and f(5000, 10, 8) < f(5000, 10, 16) < f(5000, 10, 64)
    for bad in ((0, 10, 32), (10, 0, 32), ((1 << 30) + 1, 10, 32), (10, (1 << 20) + 1, 32), (10, 10, 0), (10, 10, 4), (10, 10, 72), (10, 10, 12)):
        assert f(*bad) == 0, bad


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_raw_calls_refuse_before_any_c_call():
    import gmm

    x = torch.zeros(10, 16)
    tab, cst = torch.zeros(3, 32), torch.zeros(3)
    for name, call in (("loglik", lambda: gmm.loglik(x, tab, cst)),
                       ("posteriors", lambda: gmm.posteriors(x, tab, cst, torch.zeros(10))),
                       ("accumulate", lambda: gmm.accumulate(x, torch.zeros(10, 3))),
                       ("estep", lambda: gmm.estep(x, {"weights": np.ones(3) / 3, "means": np.zeros((3, 16)), "variances": np.ones((3, 16))}))):
        with pytest.raises(RuntimeError, match="no CPU fallback") as e:
            call()
        assert name in str(e.value) or name == "estep"
    model = {"weights": np.zeros(3), "means": np.zeros((3, 16)), "variances": np.ones((3, 16))}
    with pytest.raises(RuntimeError, match="table.*not all 0"):
        gmm.table(model)
    with pytest.raises(RuntimeError, match="table.*at most|table.*1 to 64"):
        gmm.table({"weights": np.ones(3) / 3, "means": np.zeros((3, 65)), "variances": np.ones((3, 65))})
    with pytest.raises(RuntimeError, match="table.*float64"):
        gmm.table({"weights": np.ones(3, np.float32) / 3, "means": np.zeros((3, 8)), "variances": np.ones((3, 8))})
    with pytest.raises(RuntimeError, match="table.*positive"):
        gmm.table({"weights": np.ones(3) / 3, "means": np.zeros((3, 8)), "variances": np.zeros((3, 8))})


# --------------------------------------------------------------------------------------------------------------------- CLI
def test_command_line_argument_errors(tmp_path, capsys):
    import fit_gmm as FG

    base = ["--feat-scp", str(tmp_path / "f.scp"), "--len-scp", str(tmp_path / "l.scp"), "--out", str(tmp_path / "o")]
    ck = ["--checkpoint", str(tmp_path / "c.tar")]
    for extra in (ck, ck + ["--k", "4", "--model", str(tmp_path / "m.npz")], ck + ["--k", "0"], ck + ["--k", "4", "--iters", "0"],
                  ck + ["--k", "4", "--var-floor", "0"], ["--k", "4", "--on", "feats", "--compute-dtype", "bf16"]):
        with pytest.raises(SystemExit) as e:
            FG.parse_args(base + extra)
        assert e.value.code == 2, extra
    capsys.readouterr()
    for extra in (["--k", "4"], ["--k", "4", "--on", "z1"], ["--model", "m.npz"]):
        with pytest.raises(SystemExit) as e:
            FG.parse_args(base + extra)
        err = capsys.readouterr().err
        assert e.value.code == 2 and "--checkpoint" in err and "--on" in err, extra
    _, args = FG.parse_args(base + ["--k", "4", "--on", "feats"])
    assert args.checkpoint is None and args.iters == 50 and args.tol == 1e-4 and args.seed == 0 and args.var_floor == 0.01
    assert args.kmeans_iters == 10 and args.post_out is None and args.out_format == "kaldi" and args.model is None
    _, args = FG.parse_args(base + ck + ["--model", "m.npz", "--post-out", "p", "--out-format", "numpy"])
    assert args.on == "z1" and args.k is None and args.model == "m.npz" and args.post_out == "p"
    opts = {a.dest for a in FG.build_parser()._actions}
    assert {"checkpoint", "feat_scp", "len_scp", "data_format", "mvn_path", "out", "k", "model", "on", "iters", "tol", "seed", "var_floor",
            "kmeans_iters", "batch_size", "compute_dtype", "post_out", "out_format", "item", "frame_shift", "frame_offset"} <= opts
