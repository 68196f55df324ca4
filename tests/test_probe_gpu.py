"""The frame probe on the GPU: fhvae_probe_rows / fhvae_probe_grad against the float64 oracle of tests/probe_ref.py under the bounds
derived there, the tie rule, row independence, unlabelled and NaN rows and the agreement of the two passes' logits (bitwise);
probe.fit on blobs; probe_latents.py end to end and the "probe" block of eval_model.py."""
import functools
import json

import numpy as np
import pytest
import torch

import probe_ref as R
from test_units_gpu import dev_rows, tiny_corpus

pytestmark = pytest.mark.gpu

ROWS_N = (1, 63, 64, 255, 256, 257, 700)
ROWS_C = (1, 2, 15, 16, 17, 63, 64, 65, 130)
WIDE = ((63, 17), (257, 65), (700, 130), (700, 1))
GRAD_N = (1, 1023, 1024, 1025, 2500)
GRAD_C = (1, 17, 65, 130, 300)  # one, two and four tiles of 16 classes per wave; 300: a second block of classes
#: (N, C, D) -> seed, where seed 0 leaves more than 1 % of a case's rows within 2 max E of a tie (found with the oracle alone, on
#: the CPU)
SEEDS = {}
U = R.U
WORST = {}  # the largest observed share of each bound, printed by the last test of the file


@pytest.fixture(scope="module")
def probe():
    import build_ext

    build_ext.build(verbose=False)
    import probe

    assert torch.cuda.is_available()
    probe.load_library()
    return probe


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    return a.view(np.int32) if a.dtype.itemsize == 4 else a.view(np.int64)


def share(name, err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    WORST[name] = max(WORST.get(name, 0.0), float(np.max(s)))
    return float(np.max(s))


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def case(N, C, D):
    """The inputs of probe_ref.case and what the oracle says of them, computed once."""
    x, y, tab, cst = R.case(N, C, D, SEEDS.get((N, C, D), 0))
    return x, y, tab, cst, R.forward(x, y, tab, cst)


def run_rows(probe, x, y, tab, cst, pad=4):
    return probe.rows(dev_rows(x, pad=pad), to_dev(y), to_dev(tab), to_dev(cst))


def check_rows(probe, N, C, D):
    x, y, tab, cst, f = case(N, C, D)
    near = f["gap"] <= 2 * f["Emax"]
    assert near.sum() <= 0.01 * N, "the case itself: %d of %d rows lie within 2 max E of a tie" % (near.sum(), N)
    lse, pred, nll, totals = (t.cpu().numpy() for t in run_rows(probe, x, y, tab, cst))
    lab = f["labelled"]
    s = share("lse", np.abs(lse.astype(np.float64) - f["lse"]), f["B_lse"])
    assert s <= 1.0, (N, C, D, s)
    assert not nll[~lab].any()
    if lab.any():
        s = share("nll", np.abs(nll.astype(np.float64) - f["nll"])[lab], f["B_nll"][lab])
        assert s <= 1.0, (N, C, D, s)
    assert pred.dtype == np.int32 and pred.min() >= 0 and pred.max() < C
    assert np.all(f["l"][np.arange(N), pred] >= f["l"].max(axis=1) - 2 * f["Emax"]), (N, C, D)
    assert np.array_equal(pred[~near], f["pred"][~near]), (N, C, D)
    assert totals.dtype == np.float64 and totals[1] == f["totals"][1] and abs(totals[2] - f["totals"][2]) <= near.sum()
    assert totals[2] == float((lab & (pred == y)).sum())
    dev_sum = nll.astype(np.float64).sum()
    assert abs(totals[0] - dev_sum) <= 1e-12 * max(dev_sum, 1.0) and abs(totals[0] - f["totals"][0]) <= f["B_nll"].sum() * (1 + 1e-9) + 1e-300


# ------------------------------------------------------------------------------------------------------------------- rows
@pytest.mark.parametrize("N", ROWS_N)
def test_rows_against_the_oracle(probe, N):
    for C in ROWS_C:
        check_rows(probe, N, C, 32)


@pytest.mark.parametrize("D", [8, 16, 39, 80, 128])
def test_rows_at_other_widths(probe, D):
    for N, C in WIDE:
        check_rows(probe, N, C, D)


def test_rows_with_more_class_tiles_than_one_workgroup_holds_at_once(probe):
    check_rows(probe, 300, 1000, 32)


def test_nothing_labelled(probe):
    x, y, tab, cst, f = case(257, 17, 32)
    none = np.full(257, -1, dtype=np.int32)
    lse, pred, nll, totals = run_rows(probe, x, none, tab, cst)
    assert not totals.cpu().numpy().any() and not nll.cpu().numpy().any()
    assert np.all(np.abs(lse.cpu().numpy() - f["lse"]) <= f["B_lse"])
    grad = probe.gradient(dev_rows(x), to_dev(none), to_dev(tab), to_dev(cst), lse).cpu().numpy()
    assert grad.shape == (17, 33) and grad.dtype == np.float64 and not grad.any() and not np.signbit(grad).any()
    value, g = probe.objective(dev_rows(x), to_dev(none), np.ones((17, 33)), 0.1)
    assert value == 0.0 and not g.any()


def test_labels_may_be_int64_and_any_value_outside_the_classes_is_unlabelled(probe):
    x, y, tab, cst, _ = case(257, 17, 32)
    a = run_rows(probe, x, y, tab, cst)
    y2 = y.astype(np.int64)
    y2[y < 0] = -5
    b = probe.rows(dev_rows(x), to_dev(y2), to_dev(tab), to_dev(cst))
    for u, v in zip(a, b):
        assert np.array_equal(bits(u), bits(v))


def test_raw_calls_refuse_device_tensors_they_cannot_take(probe):
    x, y = torch.zeros(10, 16, device="cuda"), torch.zeros(10, dtype=torch.int32, device="cuda")
    tab, cst = torch.zeros(3, 16, device="cuda"), torch.zeros(3, device="cuda")
    with pytest.raises(RuntimeError, match="float32"):
        probe.rows(x.double(), y, tab, cst)
    with pytest.raises(RuntimeError, match="at most 128"):
        probe.rows(torch.zeros(10, 129, device="cuda"), y, tab, cst)
    with pytest.raises(RuntimeError, match="class 3.*3 classes"):
        probe.rows(x, y + 3, tab, cst)
    with pytest.raises(RuntimeError, match="class 5"):
        probe.gradient(x, y + 5, tab, cst, torch.zeros(10, device="cuda"))
    with pytest.raises(RuntimeError, match="y must be"):
        probe.rows(x, y[:9], tab, cst)
    with pytest.raises(RuntimeError, match="tab"):
        probe.rows(x, y, torch.zeros(3, 32, device="cuda"), cst)


def test_table_is_the_oracles(probe):
    rng = np.random.default_rng(4)
    for C, D in ((17, 32), (5, 39), (130, 13)):
        w, b = rng.standard_normal((C, D)), rng.standard_normal(C)
        mean, std = rng.standard_normal(D), np.exp(rng.standard_normal(D))
        tab, cst = probe.table(w, b, mean, std)
        want_tab, want_cst = R.table(w, b, mean, std)
        assert tab.dtype == torch.float32 and tuple(tab.shape) == want_tab.shape == (C, R.padded(D)) and tab.is_cuda and tuple(cst.shape) == (C,)
        got_tab, got_cst = tab.cpu().numpy(), cst.cpu().numpy()
        assert not got_tab[:, D:].any()
        # (float64 on both sides, rounded once: a last-place difference of the two libraries' division and sum at the most)
        assert np.allclose(got_tab, want_tab, rtol=2.0 ** -23, atol=0)
        assert np.all(np.abs(got_cst - want_cst) <= 2.0 ** -23 * (np.abs(b) + (np.abs(w / std * mean)).sum(axis=1)))
    plain = probe.table(w, b)
    assert np.array_equal(plain[0].cpu().numpy()[:, :D], w.astype(np.float32)) and np.array_equal(plain[1].cpu().numpy(), b.astype(np.float32))


# --------------------------------------------------------------------------------------------------------------- gradient
def check_grad(probe, N, C, D):
    x, y, tab, cst, f = case(N, C, D)
    xd, yd, tabd, cstd = dev_rows(x), to_dev(y), to_dev(tab), to_dev(cst)
    lse = probe.rows(xd, yd, tabd, cstd)[0]
    grad = probe.gradient(xd, yd, tabd, cstd, lse).cpu().numpy()
    want, bound = R.grad(x, y, tab, cst, f)
    W = tab.shape[1]
    assert grad.shape == want.shape == (C, W + 1) and grad.dtype == np.float64
    assert not grad[:, D:W].any()
    s = share("grad", np.abs(grad - want), bound)
    assert s <= 1.0, (N, C, D, s)
    s = share("grad bias", np.abs(grad - want)[:, W], bound[:, W])
    return grad


@pytest.mark.parametrize("N", GRAD_N)
def test_gradient_against_the_oracle(probe, N):
    for C in GRAD_C:
        check_grad(probe, N, C, 32)


@pytest.mark.parametrize("D", [8, 16, 39, 80, 128])
def test_gradient_at_other_widths(probe, D):
    for N, C in ((1025, 17), (1025, 130), (700, 300)):
        check_grad(probe, N, C, D)


def test_both_passes_twice(probe):
    x, y, tab, cst, _ = case(2500, 65, 32)
    xd, yd, tabd, cstd = dev_rows(x), to_dev(y), to_dev(tab), to_dev(cst)
    a, b = probe.rows(xd, yd, tabd, cstd), probe.rows(xd, yd, tabd, cstd)
    for u, v in zip(a, b):
        assert np.array_equal(bits(u), bits(v))
    g1, g2 = probe.gradient(xd, yd, tabd, cstd, a[0]), probe.gradient(xd, yd, tabd, cstd, a[0])
    assert np.array_equal(bits(g1), bits(g2))


# ---------------------------------------------------------------------------------------------------------------- bitwise
def test_a_row_does_not_depend_on_its_batch(probe):
    x, y, tab, cst, _ = case(700, 65, 32)
    tabd, cstd = to_dev(tab), to_dev(cst)
    whole = probe.rows(dev_rows(x), to_dev(y), tabd, cstd)
    for part in (probe.rows(dev_rows(x)[100:400], to_dev(y[100:400]), tabd, cstd),
                 probe.rows(dev_rows(x[100:400], pad=12), to_dev(y[100:400]), tabd, cstd)):
        for u, v in zip(part[:3], whole[:3]):
            assert np.array_equal(bits(u), bits(v[100:400]))


@pytest.mark.parametrize("source, copies", [(5, (9, 40, 100)), (127, (115, 70, 9))])
def test_equal_classes_have_equal_logits_and_the_smallest_index_wins(probe, source, copies):
    """copies of one class in the same block of 16, in another block and in another class block of 64: bitwise equal table rows,
    so bitwise equal logits (seen through nll with that class as the label, and through the class's gradient row when no row
    carries either label), and the rows that class wins get the smallest of the four indices"""
    rng = np.random.default_rng(11)
    C, D, N = 130, 32, 300
    x, y, tab, cst = R.case(N, C, D)
    tab, cst = tab.copy(), cst.copy()
    for c in copies:
        tab[c], cst[c] = tab[source], cst[source]
    four = sorted((source,) + tuple(copies))
    assert source // 16 == copies[0] // 16 and source // 16 != copies[1] // 16 and source // 64 != copies[2] // 64
    mine = rng.permutation(N)[:60]
    x = x.copy()
    x[mine] = (16.0 * tab[source][:D] / np.linalg.norm(tab[source]) + 0.01 * rng.standard_normal((60, D))).astype(np.float32)
    f = R.forward(x, y, tab, cst)
    assert np.all(np.isin(f["pred"][mine], four))  # (the oracle: these rows are the class's)
    xd, tabd, cstd = dev_rows(x), to_dev(tab), to_dev(cst)
    ref = probe.rows(xd, to_dev(np.full(N, source, np.int32)), tabd, cstd)
    pred = ref[1].cpu().numpy()
    assert np.all(pred[mine] == four[0]) and not np.isin(pred, four[1:]).any()
    for c in copies:
        got = probe.rows(xd, to_dev(np.full(N, c, np.int32)), tabd, cstd)
        assert np.array_equal(bits(got[2]), bits(ref[2])) and np.array_equal(bits(got[0]), bits(ref[0]))
    other = np.where(np.isin(y, four), -1, y).astype(np.int32)
    grad = probe.gradient(xd, to_dev(other), tabd, cstd, ref[0]).cpu().numpy()
    for c in copies:
        assert np.array_equal(bits(grad[c]), bits(grad[source])) and grad[c].any()


def test_a_nan_row(probe):
    """rows: it poisons itself (lse NaN, pred 0, nll NaN if labelled) and the nll total, nothing else.  gradient: a labelled NaN
    row makes every entry NaN; an unlabelled one changes nothing."""
    x, y, tab, cst, _ = case(257, 65, 32)
    y = y.copy()
    y[37] = 3
    clean = x.copy()
    clean[37] = 0.0
    bad = clean.copy()
    bad[37, 5] = np.nan
    a, b = run_rows(probe, clean, y, tab, cst), run_rows(probe, bad, y, tab, cst)
    lse_b, nll_b = b[0].cpu().numpy(), b[2].cpu().numpy()
    assert np.isnan(lse_b[37]) and int(b[1][37]) == 0 and np.isnan(nll_b[37]) and np.isfinite(a[0].cpu().numpy()).all()
    others = np.arange(257) != 37
    for u, v in zip(a[:3], b[:3]):
        assert np.array_equal(bits(u)[others], bits(v)[others])
    tb = b[3].cpu().numpy()
    assert np.isnan(tb[0]) and np.array_equal(tb[1:], a[3].cpu().numpy()[1:])
    tabd, cstd = to_dev(tab), to_dev(cst)
    assert np.isnan(probe.gradient(dev_rows(bad), to_dev(y), tabd, cstd, b[0]).cpu().numpy()).all()
    y2 = y.copy()
    y2[37] = -1
    g_clean = probe.gradient(dev_rows(clean), to_dev(y2), tabd, cstd, a[0])
    g_bad = probe.gradient(dev_rows(bad), to_dev(y2), tabd, cstd, b[0])
    assert np.isfinite(g_clean.cpu().numpy()).all() and np.array_equal(bits(g_clean), bits(g_bad))
    assert int(run_rows(probe, bad, y2, tab, cst)[2][37].view(torch.int32)) == 0  # (unlabelled: nll 0 even for a NaN row)


def test_gradient_ignores_what_unlabelled_rows_hold(probe):
    x, y, tab, cst, _ = case(2500, 130, 32)
    xd, yd, tabd, cstd = dev_rows(x), to_dev(y), to_dev(tab), to_dev(cst)
    lse = probe.rows(xd, yd, tabd, cstd)[0]
    want = probe.gradient(xd, yd, tabd, cstd, lse)
    junk = x.copy()
    off = np.nonzero(y < 0)[0]
    assert 100 < off.size < 500
    junk[off[0::4]], junk[off[1::4]], junk[off[2::4]], junk[off[3::4]] = 1e30, np.nan, np.inf, -7.0
    lse2 = lse.clone()
    lse2[to_dev(off)] = float("nan")
    got = probe.gradient(dev_rows(junk), yd, tabd, cstd, lse2)
    assert np.array_equal(bits(got), bits(want))


def test_the_two_passes_use_the_same_logits(probe):
    """One-hot rows, one row per column, one class block: l(n, c) = cst[c] + tab[c][d(n)] is one f32 addition the host repeats
    exactly, and grad[c][d(n)] is the residual r(n, c) itself (a chain of one term).  With logits near 1024 one ulp of a logit is
    2^-13, so a pass whose logit differed in the last place would give a posterior off by a factor exp(2^-13), far above the
    2^-20 allowed for the device's expf below."""
    rng = np.random.default_rng(21)
    W, C = 32, 40
    x = np.eye(W, dtype=np.float32)
    tab = rng.standard_normal((C, W)).astype(np.float32)
    cst = (1024.0 + rng.standard_normal(C)).astype(np.float32)
    y = (np.arange(W) % C).astype(np.int32)
    l = cst[None, :] + tab.T  # (f32 + f32: one rounding, as the kernels)
    assert l.dtype == np.float32 and l.shape == (W, C)
    xd, tabd, cstd = to_dev(x), to_dev(tab), to_dev(cst)
    lse, pred, nll, _ = probe.rows(xd, to_dev(y), tabd, cstd)
    lse_h, nll_h = lse.cpu().numpy(), nll.cpu().numpy()
    rows = np.arange(W)
    assert np.array_equal(bits(nll_h), bits(lse_h - l[rows, y]))  # pass 1's l(n, y), bit for bit
    assert np.array_equal(pred.cpu().numpy(), l.argmax(axis=1))
    for labels in (y, ((y + 7) % C).astype(np.int32)):
        grad = probe.gradient(xd, to_dev(labels), tabd, cstd, lse).cpu().numpy()
        r = grad[:, :W].T  # r[n][c]
        assert np.array_equal(r.astype(np.float32).astype(np.float64), r)  # each entry is one f32
        p = r.copy()
        p[rows, labels] += 1.0
        want = np.exp(l.astype(np.float64) - lse_h.astype(np.float64)[:, None])
        assert np.all(np.abs(p - want) <= 2.0 ** -20 * want + 2.0 ** -23 * (np.arange(C)[None, :] == labels[:, None])), np.max(np.abs(p - want) / want)
        if labels is y:  # ... and it is pass 1's: p(n, y) = expf(-nll)
            assert np.all(np.abs(p[rows, y] - np.exp(-nll_h.astype(np.float64))) <= 2.0 ** -20 + 2.0 ** -23)
            first = r
        else:  # the same class with and without the label: r = p - 1 in f32 of the same p
            assert np.array_equal(bits((r[rows, y].astype(np.float32) - np.float32(1.0))), bits(first[rows, y].astype(np.float32)))
        assert np.allclose(grad[:, W], r.sum(axis=0), rtol=0, atol=1e-5)


# --------------------------------------------------------------------------------------------------------------------- fit
def test_fit_on_blobs(probe):
    x, y = R.blobs(600, C=5, D=8)
    y = y.copy()
    y[::13] = -1
    xd, yd = dev_rows(x), to_dev(y)
    model, hist = probe.fit(xd, yd, 5)
    assert set(model) == {"weights", "bias", "mean", "std", "classes"} and all(v.dtype == np.float64 for v in model.values())
    assert model["weights"].shape == (5, 8) and model["classes"].tolist() == [0, 1, 2, 3, 4]
    assert set(hist) == {"objective", "iterations", "converged", "evaluations", "gradient_norm"}
    assert hist["converged"] and 1 <= hist["iterations"] <= 200 and len(hist["objective"]) == hist["iterations"] + 1
    again, hist2 = probe.fit(xd, yd, 5)
    assert hist2 == hist
    for k in model:
        assert np.array_equal(bits(model[k]), bits(again[k]))
    # the float64 oracle's gradient at the returned model, through the same f32 table: gtol plus the gradient's own bound
    params = np.concatenate([model["weights"], model["bias"][:, None]], axis=1)
    value, g, b = R.objective(params, x, y, 1e-4, model["mean"], model["std"], f32=True, with_bound=True)
    assert np.all(np.abs(g) <= 1e-5 + b), float(np.max(np.abs(g) - b))
    share("fit gradient (of gtol + bound)", np.abs(g), 1e-5 + b)
    assert abs(value - hist["objective"][-1]) <= 1e-5
    lab = y >= 0
    xs = x[lab].astype(np.float64)
    assert np.allclose(model["mean"], xs.mean(axis=0), rtol=1e-12, atol=1e-14) and np.allclose(model["std"], xs.std(axis=0), rtol=1e-12)
    # score: the oracle's, exactly where no row lies within the gap
    tab, cst = R.table(model["weights"], model["bias"], model["mean"], model["std"])
    f = R.forward(x, y, tab, cst)
    assert not (f["gap"] <= 2 * f["Emax"]).any()
    got, want = probe.score(xd, yd, model), R.score(x, y, tab, cst)
    assert got["frames"] == want["frames"] == lab.sum() and np.array_equal(got["confusion"], want["confusion"])
    assert got["accuracy"] == want["accuracy"] > 0.95 and got["balanced_accuracy"] == pytest.approx(want["balanced_accuracy"], rel=1e-14)
    assert abs(got["loss"] - want["loss"]) <= f["B_nll"].sum() / lab.sum()
    # a class without a training row keeps weights 0 unless strict
    wide, _ = probe.fit(xd, yd, 6, iters=5)
    assert not wide["weights"][5].any() and wide["bias"][5] == -np.inf and np.isfinite(wide["bias"][:5]).all()
    assert not probe.score(xd, yd, wide)["confusion"][:, 5].any()
    with pytest.raises(ValueError, match="class 5"):
        probe.fit(xd, yd, 6, strict=True)
    with pytest.raises(ValueError, match="no row"):
        probe.fit(xd, to_dev(np.full(3000, -1, np.int32)), 5)


# --------------------------------------------------------------------------------------------------------------------- CLI
JSON_KEYS = ["on", "target", "classes", "train_frames", "test_frames", "unlabelled", "overlaps", "accuracy", "balanced_accuracy", "majority",
             "train_accuracy", "loss", "iterations", "converged", "l2"]


def test_probe_latents_cli_without_a_checkpoint(probe, tmp_path, capsys):
    import probe_latents as PL
    from test_gmm_gpu import feats_corpus

    base, keys, lens = feats_corpus(tmp_path)
    item = str(tmp_path / "t.item")
    out = tmp_path / "fit"
    common = base + ["--item", item, "--on", "feats", "--iters", "30"]
    assert PL.main(common + ["--out", str(out)]) == 0
    assert sorted(p.name for p in out.iterdir()) == ["confusion.tsv", "probe.json", "probe.npz"]
    info = json.load(open(out / "probe.json"))
    assert list(info) == JSON_KEYS and info["on"] == "feats" and info["target"] == "phone" and info["classes"] == ["p0", "p1", "p2", "p3"]
    assert info["train_frames"] + info["test_frames"] + info["unlabelled"] == sum(lens) and info["test_frames"] > 0 and info["l2"] == 1e-4
    assert 0.0 <= info["majority"] <= info["accuracy"] <= 1.0 and info["accuracy"] > 0.9 and info["train_accuracy"] > 0.9 and info["loss"] > 0
    assert 1 <= info["iterations"] <= 30
    lines = (out / "confusion.tsv").read_text().splitlines()
    assert lines[0].split("\t")[1:] == info["classes"] and len(lines) == 5
    assert sum(int(v) for line in lines[1:] for v in line.split("\t")[1:]) == info["test_frames"]
    model = probe.load(str(out / "probe.npz"))
    assert model["weights"].shape == (4, 13)
    # --model: the same scores without a fit, the model byte for byte
    again = tmp_path / "apply"
    assert PL.main(common + ["--out", str(again), "--model", str(out / "probe.npz")]) == 0
    applied = json.load(open(again / "probe.json"))
    assert applied["iterations"] == 0 and applied["converged"]
    assert all(applied[k] == info[k] for k in JSON_KEYS if k not in ("iterations", "converged"))
    assert (again / "probe.npz").read_bytes() == (out / "probe.npz").read_bytes()
    assert (again / "confusion.tsv").read_bytes() == (out / "confusion.tsv").read_bytes()
    # a separate test corpus (here the same one): every frame on both sides
    sep = tmp_path / "sep"
    test_side = ["--test-feat-scp", str(tmp_path / "feats.scp"), "--test-len-scp", str(tmp_path / "len.scp")]
    assert PL.main(common + ["--out", str(sep)] + test_side) == 0
    both = json.load(open(sep / "probe.json"))
    assert both["train_frames"] == both["test_frames"] and both["accuracy"] == both["train_accuracy"]
    # speakers: one speaker only, so accuracy = majority = 1; a test corpus of another speaker is refused
    spk = tmp_path / "spk"
    assert PL.main(common + ["--out", str(spk), "--target", "speaker"]) == 0
    one = json.load(open(spk / "probe.json"))
    assert one["classes"] == ["s01"] and one["accuracy"] == one["majority"] == 1.0 and one["loss"] == 0.0
    (tmp_path / "other.item").write_text((tmp_path / "t.item").read_text().replace("s01", "s02"))
    capsys.readouterr()
    assert PL.main(common + ["--out", str(tmp_path / "no"), "--target", "speaker", "--test-item", str(tmp_path / "other.item")] + test_side) == 1
    assert "s02 never occurs in training" in capsys.readouterr().err and not (tmp_path / "no").exists()
    # a model of another shape is an error
    np.savez(str(tmp_path / "narrow.npz"), weights=np.zeros((4, 12)), bias=np.zeros(4), mean=np.zeros(12), std=np.ones(12), classes=np.arange(4.0))
    assert PL.main(common + ["--out", str(tmp_path / "no"), "--model", str(tmp_path / "narrow.npz")]) == 1


def test_probe_block_of_eval_model(probe, tmp_path):
    import eval_model as EM

    base, keys, lens = tiny_corpus(tmp_path)
    item = str(tmp_path / "t.item")
    common = base + ["--max-recon", "2"]
    plain, with_p = tmp_path / "plain", tmp_path / "with"
    assert EM.main(common + ["--out", str(plain)]) == 0
    assert EM.main(common + ["--out", str(with_p), "--probe-item", item, "--probe-iters", "20"]) == 0
    s_plain, s_with = json.load(open(plain / "summary.json")), json.load(open(with_p / "summary.json"))
    assert sorted(p.name for p in with_p.iterdir()) == sorted(p.name for p in plain.iterdir())
    assert set(s_with) == set(s_plain) | {"probe"} and "probe" not in s_plain
    assert all(s_with[k] == s_plain[k] for k in ("checkpoint", "segments", "sequences"))
    assert s_with["lower_bound_per_frame"] == pytest.approx(s_plain["lower_bound_per_frame"], rel=1e-6)  # (as tests/test_units_gpu.py)
    block = s_with["probe"]
    assert set(block) == {"phone", "speaker", "holdout", "seed", "frame_shift", "frame_offset"} and block["holdout"] == 0.2 and block["seed"] == 0
    for target, classes in (("phone", ["aa", "iy", "s"]), ("speaker", ["s01", "s02"])):
        assert set(block[target]) == {"z1", "feats"}
        for on in ("z1", "feats"):
            e = block[target][on]
            assert set(e) == set(JSON_KEYS) - {"on", "target"} and e["classes"] == classes
            assert e["train_frames"] > e["test_frames"] > 0 and 0.0 <= e["accuracy"] <= 1.0 and 0.0 <= e["majority"] <= 1.0 and e["l2"] == 1e-4
    # (the features of speaker s are N(s, 1) in every one of 16 columns: a linear probe on them separates the two)
    assert block["speaker"]["feats"]["accuracy"] > 0.95
    # a baseline archive is one more entry per target
    import fit_gmm as FG

    assert FG.main(base + ["--out", str(tmp_path / "gmm"), "--k", "4", "--on", "z1", "--post-out", str(tmp_path / "post")]) == 0
    with_b = tmp_path / "with_b"
    assert EM.main(common + ["--out", str(with_b), "--probe-item", item, "--probe-iters", "5", "--probe-target", "phone", "--probe-on", "z1",
                             "--baseline-feat-scp", str(tmp_path / "post" / "feats.scp"), "--baseline-name", "gmm"]) == 0
    block = json.load(open(with_b / "summary.json"))["probe"]
    assert set(block) == {"phone", "holdout", "seed", "frame_shift", "frame_offset"} and set(block["phone"]) == {"z1", "gmm"}
    assert block["phone"]["gmm"]["train_frames"] == block["phone"]["z1"]["train_frames"]


def test_report_the_worst_share_of_each_bound(probe):
    """(no assertion of its own: the shares asserted above, for the record of DESIGN §26)"""
    print("\nworst observed share of each bound:", json.dumps(WORST, sort_keys=True))
