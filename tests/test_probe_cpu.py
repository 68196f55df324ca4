"""The frame probe without a GPU: the oracle (tests/probe_ref.py) against central differences and at its edges, probe.minimise
driven by the oracle's objective, PROBE_SIGNATURES against include/fhvae_probe.h, the entry points' argument errors (they return
before any launch), the workspace size, the refusals of the raw calls, frame_labels, split_utterances, save / load and both
command lines' argument errors."""
import os
import re

import numpy as np
import pytest
import torch

import probe_ref as R
import ext_abi
from ext_abi import aligned as _aligned, swap as _swap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, ALIGN, LIMIT = -1, -2, -4, -5


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import probe

    return probe.load_library()


# ------------------------------------------------------------------------------------------------------------------ oracle
def test_oracle_gradient_against_central_differences():
    rng = np.random.default_rng(2)
    x, y = R.blobs(40, C=4, D=5)
    y = y.copy()
    y[::7] = -1
    mean, std = x.mean(axis=0).astype(np.float64), x.std(axis=0).astype(np.float64)
    params = 0.3 * rng.standard_normal((4, 6))
    for l2, mu, sd in ((0.0, None, None), (0.05, mean, std)):
        value, g = R.objective(params, x, y, l2, mu, sd)
        h = 1e-6
        for c in range(4):
            for d in range(6):
                e = np.zeros_like(params)
                e[c, d] = h
                num = (R.objective(params + e, x, y, l2, mu, sd)[0] - R.objective(params - e, x, y, l2, mu, sd)[0]) / (2 * h)
                assert abs(num - g[c, d]) <= 1e-8 + 1e-7 * abs(g[c, d]), (l2, c, d, num, g[c, d])
    # the softmax residuals of a labelled row sum to 0: so do the bias gradients over the classes
    assert abs(g[:, 5].sum()) < 1e-14


def test_oracle_edges():
    x, y, tab, cst = R.case(50, 6, 13)
    f = R.forward(x, y, tab, cst)
    lab = y >= 0
    assert f["labelled"].tolist() == lab.tolist() and f["totals"][1] == lab.sum() and 0 < lab.sum() < 50
    assert not f["nll"][~lab].any() and np.all(f["nll"][lab] > 0) and np.all(f["gap"] >= 0) and np.all(f["B_nll"][lab] > f["B_lse"][lab])
    G, B = R.grad(x, y, tab, cst, f)
    assert G.shape == (6, 17) and not G[:, 13:16].any() and np.all(B >= 0)
    # unlabelled rows are as if they were not there, whatever their x
    x2 = x.copy()
    x2[~lab] = 1e6
    G2, _ = R.grad(x2, y, tab, cst)
    G3, _ = R.grad(x[lab], y[lab], tab, cst)
    assert np.array_equal(G2, G) and np.allclose(G3, G, rtol=0, atol=1e-12)
    # a value outside [0, C) on either side is unlabelled
    y3 = y.copy()
    y3[~lab] = 6
    assert np.array_equal(R.forward(x, y3, tab, cst)["totals"], f["totals"])
    # nothing labelled: value 0, gradient 0, counts 0
    none = np.full(50, -1, dtype=np.int32)
    f0 = R.forward(x, none, tab, cst)
    assert not f0["totals"].any() and not f0["nll"].any() and not R.grad(x, none, tab, cst, f0)[0].any()
    value, g = R.objective(np.ones((6, 14)), x, none, 0.1)
    assert value == 0.0 and not g.any()
    # one class: lse = l, nll = 0, p = 1, the residual 0, pred 0, no runner-up
    f1 = R.forward(x, np.zeros(50, np.int32), tab[:1], cst[:1])
    assert np.all(f1["gap"] == np.inf) and not f1["pred"].any() and np.allclose(f1["nll"], 0.0, atol=1e-15) and np.allclose(f1["p"], 1.0)
    assert np.allclose(R.grad(x, np.zeros(50, np.int32), tab[:1], cst[:1], f1)[0], 0.0, atol=1e-12) and f1["totals"][2] == 50
    s = R.score(x, y, tab, cst)
    assert s["frames"] == lab.sum() and s["confusion"].sum() == lab.sum() and s["accuracy"] == f["totals"][2] / f["totals"][1]


# --------------------------------------------------------------------------------------------------------------- optimiser
def test_minimise_on_the_oracles_objective():
    import probe

    x, y = R.blobs(60, C=4, D=6, spread=1.5)
    y = y.copy()
    y[::11] = -1
    mean, std = x.mean(axis=0).astype(np.float64), x.std(axis=0).astype(np.float64)
    fun = lambda p: R.objective(p, x, y, 1e-2, mean, std)
    p, hist = probe.minimise(fun, np.zeros((4, 7)), iters=200, gtol=1e-5)
    assert hist["converged"] and hist["iterations"] < 200 and hist["gradient_norm"] <= 1e-5
    assert np.max(np.abs(fun(p)[1])) <= 1e-5 and len(hist["objective"]) == hist["iterations"] + 1
    assert hist["evaluations"] >= hist["iterations"] + 1 and hist["objective"][0] == pytest.approx(np.log(4.0))
    assert all(b <= a for a, b in zip(hist["objective"][:-1], hist["objective"][1:]))
    # a long plain gradient descent of the oracle does not get below it (at gtol = 1e-5 the objective may still lie g^2 / l2 ~
    # 1e-8 above the minimum, so the comparison is made at a gtol whose g^2 / l2 is below the 1e-12 allowed here)
    q = np.zeros((4, 7))
    for _ in range(3000):
        q = q - 0.5 * fun(q)[1]
    tight, hist_t = probe.minimise(fun, np.zeros((4, 7)), iters=400, gtol=1e-8)
    assert hist_t["converged"] and hist_t["objective"][-1] <= fun(q)[0] + 1e-12 and hist_t["objective"][-1] <= hist["objective"][-1]
    assert hist["objective"][-1] <= fun(q)[0] + 1e-10 / 1e-2
    # the same input: the same bits; iters = 0: the start
    p2, hist2 = probe.minimise(fun, np.zeros((4, 7)), iters=200, gtol=1e-5)
    assert np.array_equal(p.view(np.int64), p2.view(np.int64)) and hist2 == hist
    p0, hist0 = probe.minimise(fun, np.zeros((4, 7)), iters=0)
    assert not p0.any() and hist0["iterations"] == 0 and not hist0["converged"] and hist0["evaluations"] == 1


def test_host_objective_is_the_oracles_chain_rule():
    import probe

    rng = np.random.default_rng(8)
    x, y = R.blobs(30, C=3, D=5)
    mean, std = x.mean(axis=0).astype(np.float64), x.std(axis=0).astype(np.float64)
    params = rng.standard_normal((3, 6))
    tab, cst = R.table(params[:, :5], params[:, 5], mean, std, f32=False)
    f = R.forward(x, y, tab, cst)
    G, _ = R.grad(x, y, tab, cst, f)
    got = probe._host_objective(f["totals"][0], f["totals"][1], np.concatenate([G[:, :5], G[:, 16:]], axis=1), params, 0.03, mean, std)
    want = R.objective(params, x, y, 0.03, mean, std)
    assert got[0] == pytest.approx(want[0], rel=1e-14) and np.allclose(got[1], want[1], rtol=1e-13, atol=1e-15)
    assert probe._host_objective(0.0, 0.0, G[:, :6], params, 0.03, mean, std)[0] == 0.0


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_signatures_match_the_header():
    import hip_binding as hb
    import probe

    text = ext_abi.header_text("fhvae_probe.h")
    found = ext_abi.declared("fhvae_probe.h", "fhvae_probe_")
    assert found == probe.PROBE_SIGNATURES
    assert sorted(found) == ["fhvae_probe_grad", "fhvae_probe_rows", "fhvae_probe_ws_bytes"]
    assert not set(found) & set(hb.SIGNATURES)
    for name, value in (("SLICE", probe.PROBE_SLICE), ("MAX_W", probe.PROBE_MAX_W), ("MAX_ROWS", probe.PROBE_MAX_ROWS),
                        ("MAX_CLASSES", probe.PROBE_MAX_CLASSES)):
        assert int(re.search(r"#define FHVAE_PROBE_%s (\d+)" % name, text).group(1)) == value
    assert probe.PROBE_SLICE == R.SLICE == 1024 and probe.PROBE_MAX_ROWS == 2 ** 30 and probe.PROBE_MAX_CLASSES == 65536


def test_symbols_exported_and_the_main_header_untouched(lib):
    import hip_binding as hb
    import probe

    for name in probe.PROBE_SIGNATURES:
        assert hasattr(lib, name) and name not in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12 and len(hb.SIGNATURES) == 81  # include/fhvae_hip.h is untouched
    assert "probe" not in open(os.path.join(ROOT, "include", "fhvae_hip.h")).read().lower()


def test_rows_errors_before_any_launch(lib):
    keep, p = _aligned()
    ws = lib.fhvae_probe_ws_bytes(4, 3, 32)
    fn = lib.fhvae_probe_rows
    #       x ldx N  W  tab ldt cst C y lse pred nll totals ws ws_bytes stream
    good = [p, 32, 4, 32, p, 32, p, 3, p, p, p, p, p, p, ws, None]
    for i in (0, 4, 6, 8, 9, 10, 11, 12, 13):
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((3, 0), (3, 8), (3, 24), (3, 144), (3, -16), (1, 28), (5, 16), (2, 0), (2, -1), (7, 0), (7, -3), (14, ws - 1), (14, 0)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i, bad in ((0, p + 4), (4, p + 8), (1, 34), (5, 33), (6, p + 2), (8, p + 2), (9, p + 1), (10, p + 2), (11, p + 3), (12, p + 4), (13, p + 8)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    assert fn(*_swap(good, 2, (1 << 30) + 1)) == LIMIT and fn(*_swap(good, 7, (1 << 16) + 1)) == LIMIT
    for W in range(16, 144, 16):  # every width of the rule passes the shape checks (a misaligned pointer stops the call)
        assert fn(p + 4, W, 4, W, p, W, p, 3, p, p, p, p, p, p, lib.fhvae_probe_ws_bytes(4, 3, W), None) == ALIGN, W
    del keep


def test_grad_errors_before_any_launch(lib):
    keep, p = _aligned()
    ws = lib.fhvae_probe_ws_bytes(4, 3, 32)
    fn = lib.fhvae_probe_grad
    #       x ldx N  W  tab ldt cst C y lse grad ws ws_bytes stream
    good = [p, 32, 4, 32, p, 32, p, 3, p, p, p, p, ws, None]
    for i in (0, 4, 6, 8, 9, 10, 11):
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((3, 0), (3, 8), (3, 40), (3, 144), (1, 28), (5, 16), (2, 0), (7, 0), (12, ws - 1), (12, -5)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i, bad in ((0, p + 4), (4, p + 8), (1, 34), (5, 35), (6, p + 2), (8, p + 1), (9, p + 2), (10, p + 4), (11, p + 8)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    assert fn(*_swap(good, 2, (1 << 30) + 1)) == LIMIT and fn(*_swap(good, 7, (1 << 16) + 1)) == LIMIT
    del keep


def test_workspace_is_monotone_and_small(lib):
    import probe

    f = lib.fhvae_probe_ws_bytes
    for W in (16, 32, 80, 128):
        last = 0
        for N in (1, 2, 1023, 1024, 1025, 2500, 4096, 4097, 359280, 3592800, 1 << 30):
            v = f(N, 100, W)
            assert v > 0 and v >= last and v % 256 == 0 and v == probe.ws_bytes(N, 100, W), (N, W)
            last = v
        last = 0
        for C in (1, 2, 63, 64, 65, 1000, 1 << 16):
            v = f(100000, C, W)
            assert v > 0 and v >= last, (C, W)
            last = v
            for N in (4096, 4097, 5000, 359280, 3592800):  # far below an (N, C) f32 array: nothing of that size exists
                assert f(N, C, W) < N * C * 4, (N, C, W)
    assert f(1024, 10, 32) < f(1025, 10, 32) and f(5000, 10, 16) < f(5000, 10, 32) < f(5000, 10, 128)
    for bad in ((0, 10, 32), (10, 0, 32), ((1 << 30) + 1, 10, 32), (10, (1 << 16) + 1, 32), (10, 10, 0), (10, 10, 8), (10, 10, 144), (10, 10, 40)):
        assert f(*bad) == 0, bad


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_raw_calls_refuse_before_any_c_call():
    import probe

    x, y = torch.zeros(10, 16), torch.zeros(10, dtype=torch.int32)
    tab, cst = torch.zeros(3, 16), torch.zeros(3)
    for name, call in (("rows", lambda: probe.rows(x, y, tab, cst)),
                       ("gradient", lambda: probe.gradient(x, y, tab, cst, torch.zeros(10))),
                       ("objective", lambda: probe.objective(x, y, np.zeros((3, 17)), 0.0)),
                       ("objective", lambda: probe.fit(x, y, 3))):
        with pytest.raises(RuntimeError, match="no CPU fallback") as e:
            call()
        assert name in str(e.value)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="table.*no CPU fallback"):
            probe.table(np.zeros((3, 16)), np.zeros(3))
    with pytest.raises(RuntimeError, match="params"):
        probe.objective(x, y, np.zeros(5), 0.0)
    for bad in (0, probe.PROBE_MAX_CLASSES + 1):
        with pytest.raises(ValueError, match="n_classes"):
            probe.fit(x, y, bad)


# ------------------------------------------------------------------------------------------------------------------ labels
ITEMS = """#file onset offset #phone prev-phone next-phone speaker
u1 0.00 0.03 aa sil b s1
u1 0.03 0.05 b aa sil s1
u2 0.01 0.04 b sil aa s2
u2 0.03 0.06 iy b sil s2
u9 0.00 0.10 zz sil sil s3
"""


def test_frame_labels_for_both_columns(tmp_path):
    import abx
    import probe
    import units

    path = tmp_path / "t.item"
    path.write_text(ITEMS)
    items = abx.read_items(str(path))
    keys, lengths = ["u1", "u2"], [6, 7]
    ph, names, over = probe.frame_labels(items, keys, lengths, "phone")
    want = units.frame_phones(items, keys, lengths, 0.010, 0.0)
    assert np.array_equal(ph, want[0]) and names == want[1] == ["aa", "b", "iy"] and over == want[2]
    # (abx.frame_range: the frames whose time lies in [onset, offset], so a boundary frame goes to the first token in file order)
    assert ph.dtype == np.int32 and ph.tolist() == [0, 0, 0, 0, 1, 1, -1, 1, 1, 1, 1, 2, 2] and over == 3
    sp, snames, sover = probe.frame_labels(items, keys, lengths, "speaker")
    assert snames == ["s1", "s2"] and np.array_equal(sp >= 0, ph >= 0) and sover == over
    assert sp.dtype == np.int32 and sp.tolist() == [0] * 6 + [-1] + [1] * 6
    with pytest.raises(ValueError, match="column"):
        probe.frame_labels(items, keys, lengths, "word")
    shifted = probe.frame_labels(items, keys, lengths, "speaker", frame_shift=0.005)
    assert shifted[0].tolist() == [0] * 6 + [-1, -1] + [1] * 5  # (u2's first token now starts at frame 2: the grid is passed on)


def test_split_utterances():
    import probe

    train, test = probe.split_utterances(10, 0.25, seed=3)
    perm = np.random.RandomState(3).permutation(10)
    assert test.tolist() == sorted(perm[7:].tolist()) and train.tolist() == sorted(perm[:7].tolist()) and len(test) == 3
    assert probe.split_utterances(10, 0.25, seed=3)[1].tolist() == test.tolist()
    assert probe.split_utterances(10, 0.25, seed=4)[1].tolist() != test.tolist()
    assert [len(t) for t in probe.split_utterances(2, 0.2)] == [1, 1]
    for n, h in ((1, 0.5), (2, 0.9), (5, 0.0), (5, 1.0), (0, 0.2)):
        with pytest.raises(ValueError):
            probe.split_utterances(n, h)
    assert probe.frames_of([0, 2], [3, 4, 2]).tolist() == [0, 1, 2, 7, 8] and probe.frames_of([], [3]).shape == (0,)
    assert probe.majority([0, 1, 1, -1, 2], [1, 1, 0, -1], 3) == pytest.approx(2.0 / 3.0)


def test_confusion_and_summary():
    import probe

    y, pred = np.array([0, 0, 1, 2, -1, 2, 2]), np.array([0, 1, 1, 0, 1, 2, 2])
    conf = probe.confusion(y, pred, 4)
    assert conf.dtype == np.float64 and conf.shape == (4, 4) and conf.sum() == 6 and conf[0, 1] == 1 and conf[2, 2] == 2
    s = probe.summarise(conf, 3.0)
    assert s["accuracy"] == pytest.approx(4 / 6) and s["balanced_accuracy"] == pytest.approx((0.5 + 1.0 + 2 / 3) / 3)
    assert s["loss"] == 0.5 and s["frames"] == 6
    assert probe.summarise(np.zeros((2, 2)), 0.0)["frames"] == 0


def test_save_load_round_trip(tmp_path):
    import probe

    rng = np.random.default_rng(9)
    model = {"weights": rng.standard_normal((5, 13)), "bias": rng.standard_normal(5), "mean": rng.standard_normal(13),
             "std": np.exp(rng.standard_normal(13)), "classes": np.arange(5, dtype=np.float64)}
    path = str(tmp_path / "probe.npz")
    probe.save(path, model)
    back = probe.load(path)
    assert sorted(back) == sorted(model) and sorted(os.listdir(tmp_path)) == ["probe.npz"]
    for k in model:
        assert back[k].dtype == np.float64 and np.array_equal(back[k].view(np.int64), model[k].view(np.int64))
    probe.save(str(tmp_path / "again.npz"), back)
    assert open(path, "rb").read() == open(str(tmp_path / "again.npz"), "rb").read()
    np.savez(str(tmp_path / "bad.npz"), weights=model["weights"])
    with pytest.raises(ValueError, match="bias"):
        probe.load(str(tmp_path / "bad.npz"))
    odd = dict(model, bias=model["bias"][:4])
    np.savez(str(tmp_path / "odd.npz"), **odd)
    with pytest.raises(ValueError):
        probe.load(str(tmp_path / "odd.npz"))


# --------------------------------------------------------------------------------------------------------------------- CLI
def test_probe_latents_argument_errors(tmp_path, capsys):
    import probe_latents as PL

    base = ["--feat-scp", "f.scp", "--len-scp", "l.scp", "--item", "t.item", "--out", str(tmp_path / "o")]
    ck = ["--checkpoint", "c.tar"]
    for extra in (ck + ["--holdout", "0"], ck + ["--holdout", "1"], ck + ["--holdout", "0.2", "--test-feat-scp", "a", "--test-len-scp", "b"],
                  ck + ["--test-feat-scp", "a"], ck + ["--test-item", "x.item"], ck + ["--iters", "-1"], ck + ["--l2", "-1"],
                  ck + ["--target", "word"], ck + ["--frame-shift", "0"], ["--on", "feats", "--compute-dtype", "bf16"]):
        with pytest.raises(SystemExit) as e:
            PL.parse_args(base + extra)
        assert e.value.code == 2, extra
    capsys.readouterr()
    for extra in ([], ["--on", "z1"]):
        with pytest.raises(SystemExit) as e:
            PL.parse_args(base + extra)
        err = capsys.readouterr().err
        assert e.value.code == 2 and "--checkpoint" in err and "--on" in err, extra
    with pytest.raises(SystemExit):
        PL.parse_args(base[2:] + ck)
    _, args = PL.parse_args(base + ["--on", "feats"])
    assert args.checkpoint is None and args.holdout == 0.2 and args.seed == 0 and args.l2 == 1e-4 and args.iters == 200 and args.gtol == 1e-5
    assert args.target == "phone" and args.model is None and args.frame_shift == 0.010 and args.frame_offset == 0.0
    _, args = PL.parse_args(base + ck + ["--test-feat-scp", "a", "--test-len-scp", "b", "--target", "speaker", "--model", "m.npz"])
    assert args.holdout is None and args.on == "z1" and args.test_item is None and args.model == "m.npz"
    assert "only meaningful split" in " ".join(PL.build_parser().format_help().split())  # (--help says so of --target speaker)


def test_eval_model_keeps_its_defaults_and_refuses_bad_probe_options(capsys):
    import eval_model as EM

    args = EM.build_parser().parse_args(["--checkpoint", "c", "--out", "o"])
    assert args.probe_item is None and args.probe_target == ["phone", "speaker"] and args.probe_on == ["z1", "feats"]
    assert args.probe_holdout == 0.2 and args.probe_seed == 0 and args.probe_l2 == 1e-4 and args.probe_iters == 200
    # the former defaults, untouched
    assert args.units is None and args.units_on == ["z1", "feats"] and args.abx_item is None and args.abx_distance == "angular"
    assert args.qbe_queries is None and args.baseline_feat_scp is None and args.baseline_name is None and args.sv_bins == 4096
    assert EM.parse_args(["--checkpoint", "c", "--out", "o"]).probe_item is None
    base = ["--checkpoint", "c", "--out", "o"]
    data = ["--feat-scp", "f", "--len-scp", "l"]
    for extra in (["--probe-item", "t.item"], data + ["--probe-item", "t", "--probe-holdout", "1.0"], data + ["--probe-item", "t", "--probe-iters", "-2"],
                  data + ["--probe-item", "t", "--probe-target", "word"], data + ["--probe-item", "t", "--probe-on", "mu2"],
                  data + ["--baseline-feat-scp", "b.scp"]):
        with pytest.raises(SystemExit) as e:
            EM.parse_args(base + extra)
        assert e.value.code == 2, extra
    capsys.readouterr()
    args = EM.parse_args(base + data + ["--probe-item", "t.item", "--baseline-feat-scp", "b.scp", "--probe-target", "phone"])
    assert args.baseline_name == "mfcc" and args.probe_target == ["phone"]
