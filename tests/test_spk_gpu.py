"""The speaker back end on the GPU: fhvae_spk_project, fhvae_spk_llr_range, fhvae_spk_llr_hist and fhvae_spk_llr_trials against
the float64 oracle (tests/spk_ref.py) on the shared cases (tests/spk_cases.py), the edges of their definitions, determinism,
and fit -> score_all_pairs end to end.  That the near-edge allowance is small on every case is asserted on the CPU
(tests/test_spk_cpu.py::test_the_gpu_cases_keep_the_edges_clear)."""
import numpy as np
import pytest
import torch

import spk_cases as SC
import spk_ref as R
import sv_ref

pytestmark = pytest.mark.gpu
U = R.U
PAIRED = [n for n in SC.NAMES if SC.SPECS[n]["S"] >= 2]


@pytest.fixture(scope="module")
def sb():
    import build_ext

    build_ext.build(verbose=False)
    import spk_backend

    assert torch.cuda.is_available()
    return spk_backend


def dev(t):
    return torch.from_numpy(np.array(t)).cuda()  # (a copy: read-only arrays)


def bits(t):
    return np.ascontiguousarray(t).view(np.uint32)


def ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def cum_ge(row):
    return np.concatenate([np.cumsum(row[::-1])[::-1], [0]])


def gpu_range(sb, c, label=None):
    r = sb.llr_range(dev(c["v"]), dev(c["a"]), dev(c["label"] if label is None else label), c["c"])
    assert r.dtype == torch.float32 and tuple(r.shape) == (2, 2)
    return r.cpu().numpy()


def gpu_hist(sb, c, lo, hi, NB=None, v=None, a=None, label=None):
    h = sb.llr_hist(dev(c["v"] if v is None else v), dev(c["a"] if a is None else a), dev(c["label"] if label is None else label), c["c"],
                    lo, hi, c["NB"] if NB is None else NB)
    assert h.dtype == torch.int64 and tuple(h.shape) == (2, c["NB"] if NB is None else NB)
    return h.cpu().numpy()


def own_range(r):
    return float(r[:, 0].min()), float(r[:, 1].max())


# ------------------------------------------------------------------------------------------------------------------ project
@pytest.mark.parametrize("name", SC.NAMES)
def test_project_against_oracle(sb, name):
    """Both stages: stage 1 (centring, length normalisation where the case has it) and stage 2 (A_p, q, sqrt(p)).  y_k within
    (Din + 2) 2^-24 sum_d |A_kd| |x_d - m_d| of the oracle's, scaled by r plus 4 ulp after normalisation; a and the scaled rows
    within what these allowances give through their own formulas plus their own roundings."""
    c = SC.case(name)
    tab, ln, K = c["tab"], c["ln"], c["width"]
    x = c["x"]
    stages = [("centre", x, tab["A1"], tab["m"], ln, None, None)]
    y32 = R.project(x, tab["A1"], tab["m"], normalise=ln)[0].astype(np.float32)
    stages.append(("plda", y32, tab["A_p"], tab["m2"], False, tab["q"], tab["sqrt_p"]))
    stages.append(("plda-normalised", y32, tab["A_p"], tab["m2"], True, tab["q"], tab["sqrt_p"]))
    for what, rows, A, mean, normalise, q, scale in stages:
        out, a = sb.project(dev(rows), dev(A), dev(mean), normalise=normalise, q=None if q is None else dev(q),
                            scale=None if scale is None else dev(scale))
        out = out.cpu().numpy()
        Dp = (K + 15) // 16 * 16
        assert out.shape == (len(rows), Dp) and not out[:, K:].any() and (a is None) == (q is None)
        want, want_a, y0, bound = R.project(rows, A, mean, normalise, q, scale)
        tol = (K + 2) * U * bound
        y = y0
        if normalise:
            r = np.sqrt(K) / np.maximum(np.sqrt((y0 * y0).sum(axis=1)), 1e-30)
            y = y0 * r[:, None]
            tol = tol * r[:, None] + 4 * ulp(y)
        sc = np.ones(K) if scale is None else scale.astype(np.float64)
        tol_out = np.abs(sc) * tol + (0 if scale is None else ulp(want))
        err = np.abs(out[:, :K] - want)
        print("%s %s: largest error / allowance %.3f" % (name, what, (err / np.maximum(tol_out, 1e-300)).max()))
        assert (err <= tol_out).all()
        if q is not None:
            # a = -sum_k q_k y_k^2: 2 |y_k| tol_k from y, one rounding of each square, K + 1 of the chain
            tol_a = (q * (2 * np.abs(y) * tol + tol * tol)).sum(axis=1) + (K + 2) * U * (q * y * y).sum(axis=1)
            assert (np.abs(a.cpu().numpy() - want_a) <= tol_a).all()


@pytest.mark.parametrize("name", ["S257-w5", "S777-w24", "S1100-w128"])
def test_project_row_alone_and_in_a_batch(sb, name):
    c = SC.case(name)
    tab = c["tab"]
    y32 = R.project(c["x"], tab["A1"], tab["m"], normalise=c["ln"])[0].astype(np.float32)
    args = (dev(tab["A_p"]), dev(tab["m2"]))
    kw = dict(normalise=c["ln"], q=dev(tab["q"]), scale=dev(tab["sqrt_p"]))
    out, a = sb.project(dev(y32), *args, **kw)
    out, a = out.cpu().numpy(), a.cpu().numpy()
    for r in (0, 63, 64, c["S"] // 2, c["S"] - 1):
        o1, a1 = sb.project(dev(y32[r:r + 1]), *args, **kw)
        assert np.array_equal(bits(o1.cpu().numpy()[0]), bits(out[r])) and np.array_equal(bits(a1.cpu().numpy()), bits(a[r:r + 1])), r
    o2, a2 = sb.project(dev(y32[37:]), *args, **kw)  # (another place in the workgroup)
    assert np.array_equal(bits(o2.cpu().numpy()), bits(out[37:])) and np.array_equal(bits(a2.cpu().numpy()), bits(a[37:]))
    # a leading dimension: the padded rows of stage 1 are read in place
    wide = torch.full((c["S"], y32.shape[1] + 12), 7.0, device="cuda")
    wide[:, :y32.shape[1]] = dev(y32)
    o3, a3 = sb.project(wide[:, :y32.shape[1]], *args, **kw)
    assert np.array_equal(bits(o3.cpu().numpy()), bits(out)) and np.array_equal(bits(a3.cpu().numpy()), bits(a))


# ---------------------------------------------------------------------------------------------------------- range and hist
def test_one_row_has_no_trial(sb):
    c = SC.case("S1-w16")
    r = gpu_range(sb, c)
    assert r.tolist() == [[np.inf, -np.inf], [np.inf, -np.inf]]
    assert not gpu_hist(sb, c, -1.0, 1.0).any()


@pytest.mark.parametrize("name", PAIRED)
def test_range_against_oracle(sb, name):
    c = SC.case(name)
    r = gpu_range(sb, c)
    for cls, same in ((0, True), (1, False)):
        sel = c["same"] == same
        if not sel.any():
            assert r[cls].tolist() == [np.inf, -np.inf]
            continue
        s, worst = c["s"][sel], R.delta(c["M"][sel], c["Dp"]).max()
        print("%s class %d: min %.9g (oracle %.9g), max %.9g (oracle %.9g), allowance %.3g" % (name, cls, r[cls, 0], s.min(), r[cls, 1], s.max(), worst))
        assert abs(r[cls, 0] - s.min()) <= worst and abs(r[cls, 1] - s.max()) <= worst
    assert np.array_equal(bits(r), bits(gpu_range(sb, c)))


@pytest.mark.parametrize("name", PAIRED)
def test_histogram_against_oracle(sb, name):
    """With the kernel's own lo, hi handed to the oracle: class totals exact, every cumulative count within the oracle's
    near-edge count of that edge, the same bits for permuted rows and for a second call."""
    c = SC.case(name)
    lo, hi = own_range(gpu_range(sb, c))
    h = gpu_hist(sb, c, lo, hi)
    for cls, (s, dlt, cum, near, _) in enumerate(SC.classes(c, lo, hi)):
        assert int(h[cls].sum()) == len(s), "%s: class %d holds %d trials, the oracle %d" % (name, cls, h[cls].sum(), len(s))
        diff = np.abs(cum_ge(h[cls]) - cum)
        worst = int(np.argmax(diff - near))
        print("%s class %d: %d trials, largest |cum_gpu - cum_ref| %d, most trials near one edge %d" % (name, cls, len(s), diff.max(), near.max()))
        assert (diff <= near).all(), "%s: class %d edge %d: |%d - %d| > %d trials within delta of it" % (
            name, cls, worst, cum_ge(h[cls])[worst], cum[worst], near[worst])
    assert np.array_equal(h, gpu_hist(sb, c, lo, hi))
    perm = np.random.RandomState(c["seed"] + 100).permutation(c["S"])
    assert np.array_equal(h, gpu_hist(sb, c, lo, hi, v=c["v"][perm], a=c["a"][perm], label=c["label"][perm]))
    assert np.array_equal(h, gpu_hist(sb, c, lo, hi, v=c["v"][::-1], a=c["a"][::-1], label=c["label"][::-1]))


@pytest.mark.parametrize("NB", [64, 256, 4096, 8192])
def test_every_histogram_size_and_a_given_range(sb, NB):
    """One case at every NB, over a range wider than the scores on one side and narrower on the other (the clamp)."""
    c = dict(SC.case("S257-w5"), NB=NB)
    lo, hi = own_range(gpu_range(sb, c))
    lo, hi = float(np.float32(lo - 3.0)), float(np.float32(hi - 0.25 * (hi - lo)))
    h = gpu_hist(sb, c, lo, hi)
    for cls, (s, dlt, cum, near, _) in enumerate(SC.classes(c, lo, hi)):
        assert int(h[cls].sum()) == len(s) and (np.abs(cum_ge(h[cls]) - cum) <= near).all()
        assert near.max() <= SC.CAP * len(s)  # (from the oracle alone, for this range)
    assert h[:, NB - 1].sum() > 0 and h[:, 0].sum() == 0  # (the clamped top; nothing reaches the bins below the scores)


def test_unlabelled_rows_single_speaker_and_equal_rows(sb):
    c = SC.case("S777-w24")
    lo, hi = own_range(gpu_range(sb, c))
    lab = c["label"].copy()
    drop = np.random.RandomState(5).rand(len(lab)) < 0.3
    drop[[0, 255, 256, 511, 512, 776]] = [True, False, True, True, False, True]
    lab[drop] = -1
    h = gpu_hist(sb, c, lo, hi, label=lab)
    kept = gpu_hist(sb, c, lo, hi, v=c["v"][~drop], a=c["a"][~drop], label=c["label"][~drop])
    n = int((~drop).sum())
    assert h.sum() == n * (n - 1) // 2 and np.array_equal(h, kept)
    r, rk = gpu_range(sb, c, label=lab), sb.llr_range(dev(c["v"][~drop]), dev(c["a"][~drop]), dev(c["label"][~drop]), c["c"]).cpu().numpy()
    assert np.array_equal(bits(r), bits(rk))
    none = np.full(len(lab), -1, np.int32)
    assert not gpu_hist(sb, c, lo, hi, label=none).any() and gpu_range(sb, c, label=none).tolist() == [[np.inf, -np.inf]] * 2
    # one speaker only: every trial is a target
    one = np.full(len(lab), 3, np.int32)
    h = gpu_hist(sb, c, lo, hi, label=one)
    r = gpu_range(sb, c, label=one)
    assert h[1].sum() == 0 and h[0].sum() == 777 * 776 // 2 and r[1].tolist() == [np.inf, -np.inf] and (r[0, 0], r[0, 1]) == (np.float32(lo), np.float32(hi))
    # all rows equal: one score, hi == lo, everything in bin 0
    v, a = np.repeat(c["v"][:1], 300, axis=0), np.repeat(c["a"][:1], 300)
    lab = (np.arange(300) % 7).astype(np.int32)
    r = sb.llr_range(dev(v), dev(a), dev(lab), c["c"]).cpu().numpy()
    assert r[0, 0] == r[0, 1] == r[1, 0] == r[1, 1]
    s, M = R.scores(v, a, c["c"], np.array([0]), np.array([1]))
    assert abs(r[0, 0] - s[0]) <= R.delta(M, c["Dp"])[0]
    h = gpu_hist(sb, c, float(r[0, 0]), float(r[0, 0]), v=v, a=a, label=lab)
    same = (lab[:, None] == lab[None, :])[np.triu_indices(300, 1)]
    assert h[0, 0] == same.sum() and h[1, 0] == (~same).sum() and h[:, 1:].sum() == 0


def test_a_nan_score_is_in_neither_class(sb):
    c = SC.case("S257-w5")
    lo, hi = own_range(gpu_range(sb, c))
    v = c["v"].copy()
    v[100, 2] = np.nan
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    h = sb.llr_hist(dev(v), dev(c["a"]), dev(c["label"]), c["c"], lo, hi, c["NB"], status=status).cpu().numpy()
    assert int(status.item()) == sb.SPK_NAN
    keep = np.arange(257) != 100
    assert np.array_equal(h, gpu_hist(sb, c, lo, hi, v=c["v"][keep], a=c["a"][keep], label=c["label"][keep]))
    status.zero_()
    r = sb.llr_range(dev(v), dev(c["a"]), dev(c["label"]), c["c"], status=status).cpu().numpy()
    assert int(status.item()) == sb.SPK_NAN
    assert np.array_equal(bits(r), bits(sb.llr_range(dev(c["v"][keep]), dev(c["a"][keep]), dev(c["label"][keep]), c["c"]).cpu().numpy()))
    with pytest.raises(RuntimeError, match="NaN"):
        sb.llr_range(dev(v), dev(c["a"]), dev(c["label"]), c["c"])


# ------------------------------------------------------------------------------------------------------------------- trials
@pytest.mark.parametrize("name", ["S2-w16", "S63-w1", "S257-w5", "S777-w100", "S1100-w128"])
def test_trials_against_oracle(sb, name):
    c = SC.case(name)
    rs = np.random.RandomState(c["seed"])
    S = c["S"]
    pairs = rs.randint(0, S, size=(1000, 2)).astype(np.int32)
    pairs[:4] = [[0, 0], [0, S - 1], [S - 1, 0], [S - 1, S - 1]]
    v, a = dev(c["v"]), dev(c["a"])
    got = sb.llr_trials(v, a, c["c"], dev(pairs)).cpu().numpy()
    want, M = R.scores(c["v"], c["a"], c["c"], pairs[:, 0], pairs[:, 1])
    err, tol = np.abs(got - want), R.delta(M, c["Dp"])
    print("%s: largest error / delta %.3f" % (name, (err / tol).max()))
    assert got.dtype == np.float32 and (err <= tol).all()
    swapped = sb.llr_trials(v, a, c["c"], dev(pairs[:, ::-1].copy())).cpu().numpy()
    assert np.array_equal(bits(got), bits(swapped))
    # an index outside the rows: the status bit, NaN for that trial, nothing else changes
    bad = pairs.copy()
    bad[7], bad[500], bad[999] = [S, 0], [1 % S, -1], [2 ** 31 - 1, -2 ** 31]
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = sb.llr_trials(v, a, c["c"], dev(bad), status=status).cpu().numpy()
    assert int(status.item()) == sb.SPK_BAD_INDEX
    hit = np.zeros(1000, bool)
    hit[[7, 500, 999]] = True
    assert np.isnan(out[hit]).all() and np.array_equal(bits(out[~hit]), bits(got[~hit]))
    with pytest.raises(RuntimeError, match="outside"):
        sb.llr_trials(v, a, c["c"], dev(bad))


# --------------------------------------------------------------------------------------------------------------- end to end
def _eer_bound(tar, non, classes, k):
    (_, _, cum_t, near_t, hist_t), (_, _, cum_n, near_n, hist_n) = classes
    mass = hist_t[k - 1] / len(tar) + hist_n[k - 1] / len(non)
    return mass, mass + (near_t[k - 1] + near_t[k]) / len(tar) + (near_n[k - 1] + near_n[k]) / len(non)


@pytest.mark.parametrize("lda_dim,ln", [(None, False), (16, True)])
def test_fit_and_score_all_pairs_end_to_end(sb, lda_dim, ln):
    """fit -> score_all_pairs on the planted set.  The oracle scores the rows the device holds (project has its own test): the
    EER read off the histogram is within the crossing bin's mass plus the near-edge share of its two edges of the exact EER."""
    x, label = R.planted(5, 40, 20, 24)
    xe, le = R.planted(6, 30, 20, 24)
    be = sb.fit(x, label, lda_dim, ln)
    NB = 4096
    # ---- plda
    r = be.score_all_pairs(xe, le, n_bins=NB)
    v, a = be.transform(xe)
    v, a = v.cpu().numpy(), a.cpu().numpy()
    c32 = float(np.float32(be.c))
    i, j, same = R.trials(le)
    s, M = R.scores(v, a, c32, i, j)
    lo, hi = r["lo"], r["hi"]
    assert abs(lo - s.min()) <= R.delta(M, v.shape[1]).max() and abs(hi - s.max()) <= R.delta(M, v.shape[1]).max()
    classes = []
    for cls in (True, False):
        dlt = R.delta(M[same == cls], v.shape[1], lo, hi)
        classes.append((s[same == cls], dlt) + R.edge_counts(s[same == cls], dlt, lo, hi, NB))
    tar, non = s[same], s[~same]
    frr, far = (len(tar) - classes[0][2]) / len(tar), classes[1][2] / len(non)
    k = int(np.argmax(frr >= far))
    mass, bound = _eer_bound(tar, non, classes, k)
    exact = R.exact_eer(tar, non)
    print("plda: EER %.6f, exact %.6f, bound %.2e (crossing mass %.2e), min_dcf %.4f" % (r["eer"], exact, bound, mass, r["min_dcf"]))
    assert r["n_target"] == len(tar) and r["n_nontarget"] == len(non) and r["hist"].shape == (2, NB)
    assert abs(r["eer"] - exact) <= bound and lo <= r["threshold"] <= hi and 0.0 <= r["min_dcf"] <= 1.0
    # ---- trials: the same pairs through the trial kernel, the exact EER by sorting on the host
    t = be.score_trials(xe, np.stack([i, j], axis=1))
    assert (np.abs(t - s) <= R.delta(M, v.shape[1])).all()
    assert abs(sb.exact_eer(t, same)["eer"] - exact) <= bound
    # ---- lda: the projection, then today's cosine kernel
    rl = be.score_all_pairs(xe, le, n_bins=NB, backend="lda")
    y = be.project_lda(xe).cpu().numpy()
    cs = R.cosine_scores(y, i, j)
    tar, non = cs[same], cs[~same]
    dl = sv_ref.delta(y.shape[1])
    (cum_t, near_t, hist_t), (cum_n, near_n, hist_n) = sv_ref.edge_counts(tar, NB, dl), sv_ref.edge_counts(non, NB, dl)
    frr, far = (len(tar) - cum_t) / len(tar), cum_n / len(non)
    k = int(np.argmax(frr >= far))
    mass = hist_t[k - 1] / len(tar) + hist_n[k - 1] / len(non)
    bound = mass + (near_t[k - 1] + near_t[k]) / len(tar) + (near_n[k - 1] + near_n[k]) / len(non)
    exact = R.exact_eer(tar, non)
    print("lda: EER %.6f, exact %.6f, bound %.2e" % (rl["eer"], exact, bound))
    assert abs(rl["eer"] - exact) <= bound and (rl["lo"], rl["hi"]) == (-1.0, 1.0) and -1.0 <= rl["threshold"] <= 1.0
