"""Score normalisation on the GPU: fhvae_sn_cohort_stats, fhvae_sn_range, fhvae_sn_hist and fhvae_sn_trials against the float64
oracle (tests/snorm_ref.py) on the shared cases (tests/snorm_cases.py), the edges of their definitions, bitwise row independence,
and score_all_pairs end to end on the two-condition set.  That the near-edge allowance is small on every pairs case and that the
two-condition set shows an effect at all is asserted on the CPU (tests/test_snorm_cpu.py)."""
import numpy as np
import pytest
import torch

import snorm_cases as NC
import snorm_ref as N
import spk_cases as SC
import spk_ref as R

pytestmark = pytest.mark.gpu
U = R.U


@pytest.fixture(scope="module")
def sn():
    import build_ext

    build_ext.build(verbose=False)
    import score_norm

    assert torch.cuda.is_available()
    return score_norm


def dev(t):
    return torch.from_numpy(np.array(t)).cuda()  # (a copy: read-only arrays)


def bits(t):
    return np.ascontiguousarray(t).view(np.uint32)


def cum_ge(row):
    return np.concatenate([np.cumsum(row[::-1])[::-1], [0]])


def gpu_stats(sn, v, a, z, az, c, top, status=None):
    out = sn.cohort_stats(dev(v), dev(a), dev(z), dev(az), c, top, NC.SD_FLOOR, status=status)
    assert all(t.dtype == torch.float32 and tuple(t.shape) == (len(v),) for t in out)
    return [t.cpu().numpy() for t in out]  # mu, sd, r, thr


# ------------------------------------------------------------------------------------------------------- cohort statistics
@pytest.mark.parametrize("name", NC.STATS_NAMES)
def test_cohort_stats_against_oracle(sn, name):
    c = NC.stats_case(name)
    mu, sd, r, thr = gpu_stats(sn, c["v"], c["a"], c["z"], c["az"], c["c"], c["top"])
    sd_ref = np.maximum(c["sd"], NC.SD_FLOOR)
    tol_t, tol_m, tol_s = N.stats_bounds(c["eps"], c["mu"], sd_ref)
    e_t, e_m, e_s = np.abs(thr - c["thr"]), np.abs(mu - c["mu"]), np.abs(sd - sd_ref)
    print("%s: largest error / allowance: thr %.3f, mu %.3f, sd %.3f" % (name, (e_t / tol_t).max(), (e_m / tol_m).max(), (e_s / tol_s).max()))
    assert (e_t <= tol_t).all() and (e_m <= tol_m).all() and (e_s <= tol_s).all()
    assert np.array_equal(bits(r), bits(np.float32(1) / sd)) and (sd >= np.float32(NC.SD_FLOOR)).all()
    assert (thr <= mu + U * np.abs(mu)).all()  # (the threshold is the smallest of what the mean averages)


@pytest.mark.parametrize("kind", NC.EXACT_KINDS)
def test_cohort_stats_of_integer_scores(sn, kind):
    """Every score is exact: thr exactly, mu bitwise, sd equal or adjacent."""
    v, a, z, az, c, top = NC.exact_case(kind)
    mu, sd, r, thr = gpu_stats(sn, v, a, z, az, c, top)
    s, eps = N.cohort_scores(v, a, z, az, c)
    assert np.array_equal(s, np.round(s))
    t_ref, m_ref, s_ref = N.stats(s, top)
    s32 = np.maximum(s_ref.astype(np.float32), np.float32(NC.SD_FLOOR))
    assert np.array_equal(thr, t_ref.astype(np.float32))
    assert np.array_equal(bits(mu), bits(m_ref.astype(np.float32)))
    assert ((sd == s32) | (sd == np.nextafter(s32, np.float32(np.inf))) | (sd == np.nextafter(s32, np.float32(-np.inf)))).all()
    assert np.array_equal(bits(r), bits(np.float32(1) / sd))
    if kind == "equal":
        assert (sd == np.float32(NC.SD_FLOOR)).all() and np.array_equal(thr, mu)
    if kind == "negative":
        assert (thr < 0).all() and (mu < 0).all()
    if kind == "zero":
        assert (thr[::2] == 0).all() and (s[::2, ::3] == 0).all()  # (a zero row scores az: the threshold falls on the zeros)
    if kind == "ties":
        K = N.top_k(top, s.shape[1])
        assert ((s > t_ref[:, None]).sum(axis=1) < K).all() and ((s >= t_ref[:, None]).sum(axis=1) > K).any()


@pytest.mark.parametrize("name", ["S257-Nc64-w100-top20", "S600-Nc1000-w16-top0", "S65-Nc129-w24-top20"])
def test_a_row_gives_the_same_bits_wherever_it_stands(sn, name):
    c = NC.stats_case(name)
    S = c["S"]
    args = (c["z"], c["az"], c["c"], c["top"])
    full = gpu_stats(sn, c["v"], c["a"], *args)
    for x in (0, 63, 64, S // 2, S - 1):
        one = gpu_stats(sn, c["v"][x:x + 1], c["a"][x:x + 1], *args)
        assert all(np.array_equal(bits(o), bits(f[x:x + 1])) for o, f in zip(one, full)), x
    perm = np.random.RandomState(c["seed"]).permutation(S)
    moved = gpu_stats(sn, c["v"][perm], c["a"][perm], *args)
    assert all(np.array_equal(bits(m), bits(f[perm])) for m, f in zip(moved, full))
    part = gpu_stats(sn, c["v"][37:], c["a"][37:], *args)
    assert all(np.array_equal(bits(p), bits(f[37:])) for p, f in zip(part, full))
    # a wide leading dimension on both sides
    Dp = c["v"].shape[1]
    wv, wz = torch.full((S, Dp + 12), 7.0, device="cuda"), torch.full((c["Nc"], Dp + 20), -3.0, device="cuda")
    wv[:, :Dp], wz[:, :Dp] = dev(c["v"]), dev(c["z"])
    wide = sn.cohort_stats(wv[:, :Dp], dev(c["a"]), wz[:, :Dp], dev(c["az"]), c["c"], c["top"], NC.SD_FLOOR)
    assert all(np.array_equal(bits(w.cpu().numpy()), bits(f)) for w, f in zip(wide, full))
    # the cohort permuted: the same multiset of scores -> the same threshold; the sums run in another order
    cp = np.random.RandomState(c["seed"] + 1).permutation(c["Nc"])
    mu, sd, r, thr = gpu_stats(sn, c["v"], c["a"], c["z"][cp], c["az"][cp], c["c"], c["top"])
    sd_ref = np.maximum(c["sd"], NC.SD_FLOOR)
    _, tol_m, tol_s = N.stats_bounds(c["eps"], c["mu"], sd_ref)
    assert np.array_equal(bits(thr), bits(full[3]))
    assert (np.abs(mu - c["mu"]) <= tol_m).all() and (np.abs(sd - sd_ref) <= tol_s).all()


def test_rows_and_cohort_that_are_not_finite(sn):
    c = NC.stats_case("S257-Nc64-w100-top20")
    full = gpu_stats(sn, c["v"], c["a"], c["z"], c["az"], c["c"], c["top"])
    v = c["v"].copy()
    v[100, 2], v[256, 0] = np.nan, np.inf
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = gpu_stats(sn, v, c["a"], c["z"], c["az"], c["c"], c["top"], status=status)
    assert int(status.item()) == sn.SN_NONFINITE
    keep = np.ones(257, bool)
    keep[[100, 256]] = False
    for g, f in zip(got, full):
        assert np.isnan(g[~keep]).all() and np.array_equal(bits(g[keep]), bits(f[keep]))
    with pytest.raises(RuntimeError, match="not finite"):
        sn.cohort_stats(dev(v), dev(c["a"]), dev(c["z"]), dev(c["az"]), c["c"], c["top"])
    # a cohort row that is NaN reaches every evaluation row
    z = c["z"].copy()
    z[63, 1] = np.nan
    status.zero_()
    got = gpu_stats(sn, c["v"], c["a"], z, c["az"], c["c"], c["top"], status=status)
    assert int(status.item()) == sn.SN_NONFINITE and all(np.isnan(g).all() for g in got)
    az = c["az"].copy()
    az[0] = -np.inf
    status.zero_()
    gpu_stats(sn, c["v"], c["a"], c["z"], az, c["c"], c["top"], status=status)
    assert int(status.item()) == sn.SN_NONFINITE


# -------------------------------------------------------------------------------------------------------------------- pairs
@pytest.fixture(scope="module")
def pairs_case(sn):
    """name -> (the spk_cases case, mu, r as device tensors and as numpy): the cohort statistics come from the device."""
    made = {}

    def get(name):
        if name not in made:
            c = SC.case(name)
            z, az = NC.cohort(name)
            mu, _, r, _ = sn.cohort_stats(dev(c["v"]), dev(c["a"]), dev(z), dev(az), c["c"], NC.PAIRS[name]["top"], NC.SD_FLOOR)
            made[name] = (c, mu, r, mu.cpu().numpy(), r.cpu().numpy())
        return made[name]

    return get


def own_range(r):
    return float(r[:, 0].min()), float(r[:, 1].max())


@pytest.mark.parametrize("name", NC.PAIRS_NAMES)
def test_range_and_histogram_against_oracle(sn, pairs_case, name):
    """With the device's own mu, r and lo, hi handed to the oracle: the range within the largest Delta, class totals exact, every
    cumulative count within the oracle's near-edge count, the same bits for permuted rows and for a second call."""
    c, mu, r, mu_h, r_h = pairs_case(name)
    v, a, lab = dev(c["v"]), dev(c["a"]), dev(c["label"])
    rng = sn.norm_range(v, a, mu, r, lab, c["c"]).cpu().numpy()
    for cls, (s, dlt, _, _, _) in enumerate(NC.classes(c, mu_h, r_h, 0.0, 0.0)):
        if len(s) == 0:
            assert rng[cls].tolist() == [np.inf, -np.inf]
            continue
        print("%s class %d: min %.9g (oracle %.9g), max %.9g (oracle %.9g), allowance %.3g" % (name, cls, rng[cls, 0], s.min(), rng[cls, 1], s.max(), dlt.max()))
        assert abs(rng[cls, 0] - s.min()) <= dlt.max() and abs(rng[cls, 1] - s.max()) <= dlt.max()
    assert np.array_equal(bits(rng), bits(sn.norm_range(v, a, mu, r, lab, c["c"]).cpu().numpy()))
    lo, hi = own_range(rng)
    h = sn.norm_hist(v, a, mu, r, lab, c["c"], lo, hi, c["NB"]).cpu().numpy()
    assert h.shape == (2, c["NB"])
    for cls, (s, dlt, cum, near, _) in enumerate(NC.classes(c, mu_h, r_h, lo, hi)):
        assert int(h[cls].sum()) == len(s)
        diff = np.abs(cum_ge(h[cls]) - cum)
        print("%s class %d: %d trials, largest |cum_gpu - cum_ref| %d, most trials near one edge %d" % (name, cls, len(s), diff.max(), near.max()))
        assert (diff <= near).all()
    assert np.array_equal(h, sn.norm_hist(v, a, mu, r, lab, c["c"], lo, hi, c["NB"]).cpu().numpy())
    perm = np.random.RandomState(c["seed"] + 100).permutation(c["S"])
    p = torch.from_numpy(perm).cuda()
    assert np.array_equal(h, sn.norm_hist(v[p], a[p], mu[p], r[p], lab[p], c["c"], lo, hi, c["NB"]).cpu().numpy())
    assert np.array_equal(bits(rng), bits(sn.norm_range(v[p], a[p], mu[p], r[p], lab[p], c["c"]).cpu().numpy()))


@pytest.mark.parametrize("name", ["S63-w1", "S257-w5", "S777-w100", "S1100-w128"])
def test_trials_against_oracle(sn, pairs_case, name):
    c, mu, r, mu_h, r_h = pairs_case(name)
    S = c["S"]
    rs = np.random.RandomState(c["seed"])
    pairs = rs.randint(0, S, size=(1000, 2)).astype(np.int32)
    pairs[:4] = [[0, 0], [0, S - 1], [S - 1, 0], [S - 1, S - 1]]
    v, a = dev(c["v"]), dev(c["a"])
    got = sn.norm_trials(v, a, mu, r, c["c"], dev(pairs)).cpu().numpy()
    s, M = R.scores(c["v"], c["a"], c["c"], pairs[:, 0], pairs[:, 1])
    want = N.normalise(s, mu_h, r_h, pairs[:, 0], pairs[:, 1])
    err, tol = np.abs(got - want), N.norm_delta(s, M, c["Dp"], mu_h, r_h, pairs[:, 0], pairs[:, 1])
    print("%s: largest error / Delta %.3f" % (name, (err / tol).max()))
    assert got.dtype == np.float32 and (err <= tol).all()
    swapped = sn.norm_trials(v, a, mu, r, c["c"], dev(pairs[:, ::-1].copy())).cpu().numpy()
    assert np.array_equal(bits(got), bits(swapped))
    bad = pairs.copy()
    bad[7], bad[500], bad[999] = [S, 0], [1 % S, -1], [2 ** 31 - 1, -2 ** 31]
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = sn.norm_trials(v, a, mu, r, c["c"], dev(bad), status=status).cpu().numpy()
    assert int(status.item()) == sn.SN_BAD_INDEX
    hit = np.zeros(1000, bool)
    hit[[7, 500, 999]] = True
    assert np.isnan(out[hit]).all() and np.array_equal(bits(out[~hit]), bits(got[~hit]))
    with pytest.raises(RuntimeError, match="outside"):
        sn.norm_trials(v, a, mu, r, c["c"], dev(bad))


@pytest.mark.parametrize("name", ["S65-w16", "S777-w24", "S1100-w128"])
def test_no_normalisation_gives_the_bits_of_the_plain_score(sn, name):
    """mu = 0, r = 1: sn == s exactly, so range, histogram and trials have the bits of spk_backend's."""
    import spk_backend as sb

    c = SC.case(name)
    v, a, lab = dev(c["v"]), dev(c["a"]), dev(c["label"])
    mu, r = torch.zeros(c["S"], device="cuda"), torch.ones(c["S"], device="cuda")
    rng = sb.llr_range(v, a, lab, c["c"]).cpu().numpy()
    assert np.array_equal(bits(rng), bits(sn.norm_range(v, a, mu, r, lab, c["c"]).cpu().numpy()))
    lo, hi = own_range(rng)
    assert np.array_equal(sb.llr_hist(v, a, lab, c["c"], lo, hi, c["NB"]).cpu().numpy(), sn.norm_hist(v, a, mu, r, lab, c["c"], lo, hi, c["NB"]).cpu().numpy())
    pairs = dev(np.random.RandomState(3).randint(0, c["S"], size=(500, 2)).astype(np.int32))
    assert np.array_equal(bits(sb.llr_trials(v, a, c["c"], pairs).cpu().numpy()), bits(sn.norm_trials(v, a, mu, r, c["c"], pairs).cpu().numpy()))


def test_a_nan_normalised_score_is_in_neither_class(sn, pairs_case):
    c, mu, r, mu_h, r_h = pairs_case("S257-w5")
    v, a, lab = dev(c["v"]), dev(c["a"]), dev(c["label"])
    lo, hi = own_range(sn.norm_range(v, a, mu, r, lab, c["c"]).cpu().numpy())
    bad = mu.clone()
    bad[100] = float("nan")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    h = sn.norm_hist(v, a, bad, r, lab, c["c"], lo, hi, c["NB"], status=status).cpu().numpy()
    assert int(status.item()) == sn.SN_NAN
    keep = torch.from_numpy(np.flatnonzero(np.arange(257) != 100)).cuda()
    assert np.array_equal(h, sn.norm_hist(v[keep], a[keep], mu[keep], r[keep], lab[keep], c["c"], lo, hi, c["NB"]).cpu().numpy())
    with pytest.raises(RuntimeError, match="NaN"):
        sn.norm_range(v, a, bad, r, lab, c["c"])


# --------------------------------------------------------------------------------------------------------------- end to end
def _eer_bound(tar, non, classes, k):
    (_, _, cum_t, near_t, hist_t), (_, _, cum_n, near_n, hist_n) = classes
    mass = hist_t[k - 1] / len(tar) + hist_n[k - 1] / len(non)
    return mass, mass + (near_t[k - 1] + near_t[k]) / len(tar) + (near_n[k - 1] + near_n[k]) / len(non)


@pytest.mark.parametrize("which,top", [("plda", 0), ("plda", 200), ("cosine", 200)])
def test_score_all_pairs_on_the_two_conditions(sn, which, top):
    """fit -> score_norm.score_all_pairs on the two-condition set.  The oracle normalises the rows and with the statistics the
    device holds (they have their own tests): the EER read off the histogram is within the crossing bin's mass plus the
    near-edge share of its two edges of the oracle's exact EER, and below the raw EER of the same rows."""
    import spk_backend as sb

    d = N.two_conditions()
    NB = 4096
    be = sb.fit(*R.planted(132, 120, 20, 32, nuisance=0), None, True, 5)
    got = sn.score_all_pairs(be, d["x"], d["label"], d["cohort"], top=top, which=which, n_bins=NB)
    assert got["top"] == (600 if top == 0 else top) and got["cohort"] == 600 and got["hist"].shape == (2, NB)
    v, a, c = sn.operands(be, d["x"], which)
    z, az, _ = sn.operands(be, d["cohort"], which)
    mu, _, r, _ = sn.cohort_stats(v, a, z, az, c, top)
    v, a, mu, r = (t.cpu().numpy() for t in (v, a, mu, r))
    i, j, same = R.trials(d["label"])
    s, M = R.scores(v, a, c, i, j)
    snr = N.normalise(s, mu, r, i, j)
    lo, hi = got["lo"], got["hi"]
    worst = N.norm_delta(s, M, v.shape[1], mu, r, i, j).max()
    assert abs(lo - snr.min()) <= worst and abs(hi - snr.max()) <= worst
    classes = []
    for cls in (True, False):
        sel = same == cls
        dlt = N.norm_delta(s[sel], M[sel], v.shape[1], mu, r, i[sel], j[sel], lo, hi)
        classes.append((snr[sel], dlt) + R.edge_counts(snr[sel], dlt, lo, hi, NB))
    tar, non = snr[same], snr[~same]
    frr, far = (len(tar) - classes[0][2]) / len(tar), classes[1][2] / len(non)
    k = int(np.argmax(frr >= far))
    mass, bound = _eer_bound(tar, non, classes, k)
    exact, raw = R.exact_eer(tar, non), R.exact_eer(s[same], s[~same])
    print("%s top %d: EER %.6f, exact %.6f, bound %.2e (crossing mass %.2e), raw %.6f" % (which, top, got["eer"], exact, bound, mass, raw))
    assert got["n_target"] == len(tar) and got["n_nontarget"] == len(non)
    assert abs(got["eer"] - exact) <= bound and lo <= got["threshold"] <= hi
    assert got["eer"] < raw
    # the same pairs through the trial kernel
    sub = np.random.RandomState(1).choice(len(i), 5000, replace=False)
    t = sn.score_trials(be, d["x"], np.stack([i[sub], j[sub]], axis=1), d["cohort"], top=top, which=which)
    assert (np.abs(t - snr[sub]) <= N.norm_delta(s[sub], M[sub], v.shape[1], mu, r, i[sub], j[sub])).all()
