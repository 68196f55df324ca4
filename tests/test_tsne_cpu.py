"""t-SNE without a GPU: the oracle's own sanity (tests/tsne_ref.py), scikit-learn's exact t-SNE as a second witness, the host-side
refusals of fhvae_tsne_* and the option rules of tsne.py and eval_model.py."""
import ctypes

import numpy as np
import pytest

import tsne_ref as R


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding as hb

    return hb.load_library()


@pytest.fixture(scope="module")
def small():
    X, label = R.make_case(120, 16, 5, 0)  # (seed 0: two duplicated rows)
    d2 = R.sqdist(R.center(X))
    beta, m, Z = R.affinity(d2, 10.0)
    return X, label, d2, beta, m, Z, R.joint_p(d2, beta, m, Z)


def test_oracle_affinities(small):
    X, _, d2, beta, m, Z, P = small
    assert (X[60] == X[3]).all() and m[3] == 0.0 and m[60] == 0.0
    assert abs(P.sum() - 1.0) <= 1e-12 and np.array_equal(P, P.T) and (np.diag(P) == 0).all() and (P >= 0).all()
    perp = np.exp(R.entropy(d2, beta))
    print("largest |perplexity / 10 - 1| of the float64 oracle: %.2e" % np.abs(perp / 10.0 - 1.0).max())
    assert np.abs(perp / 10.0 - 1.0).max() <= 1e-12
    # the three vectors are all the gradient needs: P from them alone
    assert np.array_equal(R.joint_p(d2, beta), P)
    # the float32 model follows the same definition
    b32, m32, z32 = R.affinity(R.sqdist(R.center(X), np.float32), 10.0)
    assert b32.dtype == m32.dtype == z32.dtype == np.float32
    assert np.abs(np.exp(R.entropy(d2, b32)) / 10.0 - 1.0).max() <= 1e-3


def test_oracle_gradient_is_the_derivative_of_its_kl(small):
    P = small[6]
    rs = np.random.RandomState(1)
    Y = rs.randn(P.shape[0], 2)
    g = R.gradient(P, Y)
    assert abs(g["Zq"] - g["W"].sum()) <= 1e-9 * g["Zq"]
    h = 1e-5
    for i, k in [(0, 0), (3, 1), (60, 0), (119, 1), (77, 0)]:
        Yp, Ym = Y.copy(), Y.copy()
        Yp[i, k] += h
        Ym[i, k] -= h
        num = (R.kl_divergence(P, Yp) - R.kl_divergence(P, Ym)) / (2 * h)
        assert abs(num - g["grad"][i, k]) <= 1e-7 * max(1.0, np.abs(g["grad"]).max()), (i, k, num, g["grad"][i, k])
    # the exaggeration multiplies F alone
    g12 = R.gradient(P, Y, 12.0)
    assert np.allclose(g12["F"], 12.0 * g["F"], rtol=1e-14, atol=0) and np.array_equal(g12["R"], g["R"]) and g12["kl"] == g["kl"]
    assert R.ratio(R.fast_gradient(P, Y, 12.0), g12["grad"]) <= 1e-12


def test_oracle_update_rule():
    Y = np.array([[1.0, -1.0], [0.5, 0.25]])
    V = np.array([[0.1, 0.1], [-0.2, 0.0]])
    G = np.array([[1.0, 0.01], [1.0, 1.0]])
    grad = np.array([[-1.0, 2.0], [-3.0, 4.0]])
    Y1, V1, G1 = R.update(Y, V, G, grad, 0.5, 10.0)
    assert np.array_equal(G1, [[1.2, 0.01], [0.8, 0.8]])  # V grad < 0: + 0.2; else * 0.8, floored at 0.01
    assert np.allclose(V1, 0.5 * V - 10.0 * G1 * grad, rtol=1e-15) and np.allclose(Y1, Y + V1, rtol=1e-15)
    assert R.schedule(0) == (12.0, 0.5) and R.schedule(249) == (12.0, 0.5) and R.schedule(250) == (1.0, 0.8)
    assert R.learning_rate(300) == 50.0 and R.learning_rate(4800) == 100.0


def test_sklearn_exact_tsne_is_a_second_witness():
    pytest.importorskip("sklearn")
    import inspect

    from sklearn.manifold import TSNE

    N = 300
    X, _ = R.make_case(N, 32, 6, 1)
    Xc = R.center(X)
    d2 = R.sqdist(Xc)
    P = R.joint_p(d2, *R.affinity(d2, 30.0))
    lr = R.learning_rate(N)
    Y, _, _ = R.run(P, R.y0(N, 0), 500, lr, fast=True)
    ours = R.kl_divergence(P, Y)
    iters = "max_iter" if "max_iter" in inspect.signature(TSNE.__init__).parameters else "n_iter"
    ts = TSNE(n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate=lr, init=R.y0(N, 0), method="exact",
              min_grad_norm=0.0, n_iter_without_progress=500, **{iters: 500})
    ts.fit(Xc.astype(np.float64))
    print("final KL after 500 iterations: oracle %.4f, scikit-learn %.4f" % (ours, ts.kl_divergence_))
    assert abs(ours - ts.kl_divergence_) <= 0.05 * ts.kl_divergence_


def test_host_side_refusals(lib):
    """Argument errors come back as negative codes before anything touches a GPU."""
    buf = (ctypes.c_float * 65536)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ws_ok = lib.fhvae_tsne_ws_bytes(64, 32)
    assert 0 < ws_ok <= 65536 * 4
    ok = dict(x=p, ld=32, N=64, D=32, perp=10.0, beta=p, m=p, z=p, y=p, v=p, g=p, kl=None, out=p, scal=p, ws=p, wsb=ws_ok)

    def aff(**kw):
        a = dict(ok, **kw)
        return lib.fhvae_tsne_affinity(a["x"], a["ld"], a["N"], a["D"], a["perp"], a["beta"], a["m"], a["z"], a["ws"], a["wsb"], None)

    def step(**kw):
        a = dict(ok, **kw)
        return lib.fhvae_tsne_step(a["x"], a["ld"], a["N"], a["D"], a["beta"], a["m"], a["z"], a["y"], a["v"], a["g"], 12.0, 0.5, 50.0,
                                   a["kl"], a["ws"], a["wsb"], None)

    def grad(**kw):
        a = dict(ok, **kw)
        return lib.fhvae_tsne_grad(a["x"], a["ld"], a["N"], a["D"], a["beta"], a["m"], a["z"], a["y"], 1.0, a["out"], a["scal"], a["ws"],
                                   a["wsb"], None)

    for fn, names in ((aff, ("x", "beta", "m", "z", "ws")), (step, ("x", "beta", "m", "z", "y", "v", "g", "ws")),
                      (grad, ("x", "beta", "m", "z", "y", "out", "scal", "ws"))):
        for name in names:
            assert fn(**{name: None}) == -1, (fn.__name__, name)
        assert fn(N=7) == -2                      # fewer than 8 rows
        assert fn(D=24, ld=24) == -2              # not a multiple of 16
        assert fn(D=144, ld=144) == -2            # beyond the widest instantiation
        assert fn(D=0) == -2
        assert fn(ld=16) == -2                    # ld < D
        assert fn(ld=34) == -4                    # rows not 16-byte aligned
        assert fn(x=ctypes.c_void_p(p.value + 4)) == -4
        assert fn(ws=ctypes.c_void_p(p.value + 4)) == -4
        assert fn(wsb=ws_ok - 256) == -2          # workspace too small
        assert fn(N=(1 << 22) + 1, wsb=1 << 40) == -5
    assert aff(perp=0.5) == -2 and aff(perp=float("nan")) == -2
    assert aff(perp=21.5) == -2 and aff(N=8, perp=3.0) == -2  # above (N - 1) / 3
    assert aff(beta=ctypes.c_void_p(p.value + 2)) == -4
    assert step(y=ctypes.c_void_p(p.value + 4)) == -4 and grad(y=ctypes.c_void_p(p.value + 4)) == -4
    assert step(kl=ctypes.c_void_p(p.value + 2)) == -4
    # the workspace: 0 for what the entries refuse; the norms and 7 N floats per chunk, N * chunks <= max(N, 2^19)
    assert lib.fhvae_tsne_ws_bytes(0, 32) == 0 and lib.fhvae_tsne_ws_bytes((1 << 22) + 1, 32) == 0
    for n in (8, 700, 4600, 16384, 28000, 100000, 1 << 20):
        b = lib.fhvae_tsne_ws_bytes(n, 32)
        assert b % 256 == 0 and 8 * n * 4 <= b <= (30 << 20) + 8 * n * 4, (n, b)


def test_tsne_parameter_rules():
    import tsne as T

    with pytest.raises(ValueError, match=r"perplexity 30 .*N = 60"):
        T.check_params(60, 30.0, 100)
    with pytest.raises(ValueError, match="perplexity 0.5"):
        T.check_params(60, 0.5, 100)
    with pytest.raises(ValueError, match="at least 8 rows"):
        T.check_params(7, 2.0, 100)
    with pytest.raises(ValueError, match="n_iter"):
        T.check_params(60, 5.0, 0)
    T.check_params(91, 30.0, 1)
    assert T.learning_rate(300) == R.learning_rate(300) and T.learning_rate(28000) == R.learning_rate(28000)
    assert np.array_equal(T.initial_map(50, 3), R.y0(50, 3))
    with pytest.raises(ValueError, match=r"\(N, D\)"):
        T.tsne(np.zeros(5, np.float32))
    with pytest.raises(ValueError, match=r"perplexity 30 .*N = 20"):
        T.tsne(np.zeros((20, 16), np.float32))


def test_eval_model_tsne_option_rules(capsys):
    import eval_model as EM

    base = ["--checkpoint", "c", "--out", "o"]
    with pytest.raises(SystemExit) as e:
        EM.parse_args(base + ["--tsne"])
    assert e.value.code == 2 and "--feat-scp" in capsys.readouterr().err
    for bad in (["--tsne-perplexity", "0.5"], ["--tsne-perplexity", "nan"], ["--tsne-iters", "0"], ["--tsne-seed", "-1"],
                ["--tsne-iters", "many"]):
        with pytest.raises(SystemExit) as e:
            EM.parse_args(base + ["--feat-scp", "f", "--tsne"] + bad)
        assert e.value.code == 2 and bad[0] in capsys.readouterr().err
    a = EM.parse_args(base + ["--feat-scp", "f", "--tsne"])
    assert a.tsne and a.tsne_perplexity == 30.0 and a.tsne_iters == 1000 and a.tsne_seed == 0
    a = EM.parse_args(base + ["--feat-scp", "f", "--tsne", "--tsne-perplexity", "12.5", "--tsne-iters", "300", "--tsne-seed", "7"])
    assert (a.tsne_perplexity, a.tsne_iters, a.tsne_seed) == (12.5, 300, 7)
    assert not EM.parse_args(base).tsne
