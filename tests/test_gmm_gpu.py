"""The mixture on the GPU: fhvae_gmm_loglik / fhvae_gmm_post against the float64 oracle of tests/gmm_ref.py under the bounds of
include/fhvae_gmm.h, their tie rule, row independence and edge cases (bitwise); fhvae_gmm_stats against the float64 sums of
the device's own posteriors, and its accumulate flag (bitwise); gmm.estep's chunks; gmm.fit on blobs; fit_gmm.py end to end and
its posteriorgrams through eval_model.py --baseline-feat-scp."""
import functools
import json

import numpy as np
import pytest
import torch

import gmm_ref as R
from test_units_gpu import dev_rows, tiny_corpus

pytestmark = pytest.mark.gpu

LL_N = (1, 63, 64, 255, 256, 257, 700)
LL_K = (1, 2, 15, 16, 17, 63, 64, 65, 130)
WIDE_N, WIDE_K = (63, 257, 700), (1, 17, 65, 130)
#: (N, K, D) -> seed, where seed 0 leaves more than 1 % of a case's rows within 2 max E of a tie (found with the oracle alone, on
#: the CPU)
SEEDS = {(63, 65, 32): 1}
STATS_N, STATS_K = (1, 1023, 1024, 1025, 2500), (1, 17, 65, 130)
FIT_SEED = 4  # (units.initial_rows(3000, 6, 4) draws one row of each blob: found on the CPU)
U = R.U
WORST = {}  # the largest observed share of each bound, printed by the last test of the file


@pytest.fixture(scope="module")
def gmm():
    import build_ext

    build_ext.build(verbose=False)
    import gmm

    assert torch.cuda.is_available()
    gmm.load_library()
    return gmm


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a.view(np.int64)


def share(name, err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    WORST[name] = max(WORST.get(name, 0.0), float(np.max(s)))
    return float(np.max(s))


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def post_buffer(N, K, extra=4):
    """an (N, K) view of an allocation with leading dimension ldp > K, filled with 77"""
    ldp = (K + 3) // 4 * 4 + extra
    buf = torch.full((N, ldp), 77.0, dtype=torch.float32, device="cuda")
    return buf, buf[:, :K]


@functools.lru_cache(maxsize=None)
def ll_case(N, K, D):
    """The inputs of gmm_ref.case, the f32 table the device gets and what the oracle says of them, computed once."""
    x, w, mu, var = R.case(N, K, D, SEEDS.get((N, K, D), 0))
    tab, cst = R.table(w, mu, var)
    return x, tab, cst, R.estep(x, tab, cst)


def run(gmm, x, tab, cst, with_post=True, pad=4):
    xd, tabd, cstd = dev_rows(x, pad=pad), to_dev(tab), to_dev(cst)
    ll, labels = gmm.loglik(xd, tabd, cstd)
    post = buf = None
    if with_post:
        buf, view = post_buffer(x.shape[0], tab.shape[0])
        post = gmm.posteriors(xd, tabd, cstd, ll, out=view)
        assert post.data_ptr() == view.data_ptr()
    return ll, labels, post, buf


def check_case(gmm, N, K, D, with_post=True):
    x, tab, cst, e = ll_case(N, K, D)
    near = e["gap"] <= 2 * e["Emax"]
    assert near.sum() <= 0.01 * N, "the case itself: %d of %d rows lie within 2 max E of a tie" % (near.sum(), N)
    ll, labels, post, buf = run(gmm, x, tab, cst, with_post)
    ll, labels = ll.cpu().numpy().astype(np.float64), labels.cpu().numpy()
    s = share("loglik", np.abs(ll - e["loglik"]), e["B_ll"])
    assert s <= 1.0, (N, K, D, s)
    assert labels.dtype == np.int32 and labels.min() >= 0 and labels.max() < K
    got = e["l"][np.arange(N), labels]
    assert np.all(got >= e["l"].max(axis=1) - 2 * e["Emax"]), (N, K, D)
    assert np.array_equal(labels[~near], e["labels"][~near]), (N, K, D)
    if with_post:
        p = post.cpu().numpy().astype(np.float64)
        s = share("post", np.abs(p - e["post"]), e["B_post"][:, None] * e["post"] + 2.0 ** -126)
        assert s <= 1.0, (N, K, D, s)
        s = share("post row sum", np.abs(p.sum(axis=1) - 1.0), (K + 16) * U + 2 * e["Emax"])
        assert s <= 1.0, (N, K, D, s)
        assert bool((buf[:, K:] == 77.0).all()), (N, K, D)  # ldp > K: the padding is untouched


# ------------------------------------------------------------------------------------------------------- loglik, label, post
@pytest.mark.parametrize("N", LL_N)
def test_loglik_labels_and_posteriors_against_the_oracle(gmm, N):
    for K in LL_K:
        check_case(gmm, N, K, 32)


@pytest.mark.parametrize("D", [8, 16, 39, 64])
def test_other_widths(gmm, D):
    for N in WIDE_N:
        for K in WIDE_K:
            check_case(gmm, N, K, D, with_post=(N, K) in ((63, 17), (257, 65), (700, 130), (700, 1)))


def test_table_is_the_oracles(gmm):
    for K, D in ((17, 32), (5, 39), (130, 13)):
        _, w, mu, var = R.case(10, K, D)
        w[K // 2] = 0.0
        tab, cst = gmm.table({"weights": w, "means": mu, "variances": var})
        want_tab, want_cst = R.table(w, mu, var)
        assert tab.dtype == torch.float32 and tuple(tab.shape) == want_tab.shape and tab.is_cuda and tuple(cst.shape) == (K,)
        got_tab, got_cst = tab.cpu().numpy(), cst.cpu().numpy()
        assert got_cst[K // 2] == -np.inf and np.array_equal(got_tab == 0, want_tab == 0)
        # (float64 on both sides, rounded once: a last-place difference of the two libraries' log and division at the most)
        assert np.allclose(got_tab, want_tab, rtol=2.0 ** -23, atol=0)
        keep = np.arange(K) != K // 2
        assert np.allclose(got_cst[keep], want_cst[keep], rtol=2.0 ** -23, atol=0)


@pytest.mark.parametrize("source, copies", [(5, (6, 12, 40, 100)), (127, (125, 115, 70, 9))])
def test_equal_components_have_equal_posteriors_and_the_smallest_index_wins(gmm, source, copies):
    """copies of one component in the same group of four, in the same block of 16, in another block and in another tile of 64:
    bitwise equal table rows, so bitwise equal posteriors, and the rows nearest to it get the smallest of the five indices"""
    rng = np.random.default_rng(11)
    K, D, N = 130, 32, 300
    _, w, mu, var = R.case(N, K, D)
    for c in copies:
        mu[c], var[c], w[c] = mu[source], var[source], w[source]
    x = rng.standard_normal((N, D)).astype(np.float32)
    mine = rng.permutation(N)[:60]
    x[mine] = (mu[source] + 0.01 * rng.standard_normal((60, D))).astype(np.float32)
    five = sorted((source,) + tuple(copies))
    assert source // 4 == copies[0] // 4 and source // 16 == copies[1] // 16 != copies[2] // 16 and source // 64 != copies[3] // 64
    tab, cst = R.table(w, mu, var)
    for c in copies:
        assert np.array_equal(bits(tab[c]), bits(tab[source])) and cst[c] == cst[source]
    e = R.estep(x, tab, cst)
    assert np.all(np.isin(e["labels"][mine], five))  # (the oracle: these rows are the component's)
    ll, labels, post, _ = run(gmm, x, tab, cst)
    labels, post = labels.cpu().numpy(), post.cpu().numpy()
    assert np.all(labels[mine] == five[0]) and not np.isin(labels, five[1:]).any()
    for c in copies:
        assert np.array_equal(bits(post[:, c]), bits(post[:, source]))
    # a table whose every row is the same: label 0, every posterior of a row the same
    same_tab, same_cst = np.repeat(tab[source][None, :], K, axis=0), np.repeat(cst[source], K)
    ll, labels, post, _ = run(gmm, x, same_tab, same_cst)
    post = post.cpu().numpy()
    assert not labels.any() and np.all(bits(post) == bits(post[:, :1]))
    assert np.allclose(post, 1.0 / K, rtol=1e-4)


def test_a_row_does_not_depend_on_its_batch(gmm):
    x, tab, cst, _ = ll_case(700, 65, 32)
    xd, tabd, cstd = dev_rows(x), to_dev(tab), to_dev(cst)

    def all_of(rows):
        ll, labels = gmm.loglik(rows, tabd, cstd)
        return ll, labels, gmm.posteriors(rows, tabd, cstd, ll)

    whole = all_of(xd)
    for part in (all_of(xd[100:400]), all_of(dev_rows(x[100:400], pad=12))):
        assert torch.equal(part[0].view(torch.int32), whole[0][100:400].view(torch.int32))
        assert torch.equal(part[1], whole[1][100:400])
        assert torch.equal(part[2].contiguous().view(torch.int32), whole[2][100:400].contiguous().view(torch.int32))


def test_a_component_of_weight_zero(gmm):
    N, K, D = 300, 17, 32
    x, w, mu, var = R.case(N, K, D)
    w[[0, 9]] = 0.0  # (component 0: the first a lane meets, while its running maximum is still -inf)
    w /= w.sum()
    tab, cst = R.table(w, mu, var)
    assert cst[0] == -np.inf and cst[9] == -np.inf
    e = R.estep(x, tab, cst)
    ll, labels, post, _ = run(gmm, x, tab, cst)
    ll, labels, post = ll.cpu().numpy().astype(np.float64), labels.cpu().numpy(), post.cpu().numpy()
    assert not post[:, [0, 9]].any() and not np.isin(labels, (0, 9)).any()
    assert np.all(np.abs(ll - e["loglik"]) <= e["B_ll"])
    assert np.all(np.abs(post - e["post"]) <= e["B_post"][:, None] * e["post"] + 2.0 ** -126)
    # every component but the last of weight 0
    w2 = np.zeros(K)
    w2[K - 1] = 1.0
    tab, cst = R.table(w2, mu, var)
    ll, labels, post, _ = run(gmm, x, tab, cst)
    post = post.cpu().numpy()
    assert np.all(labels.cpu().numpy() == K - 1) and np.all(post[:, K - 1] == 1.0) and not post[:, :K - 1].any()
    assert bool(torch.isfinite(ll).all())


def test_a_row_far_from_every_mean(gmm):
    N, K, D = 64, 17, 32
    x, w, mu, var = R.case(N, K, D)
    sd = np.sqrt(var.max())
    x[7] = (1e3 * sd * np.where(np.arange(D) % 2, 1.0, -1.0)).astype(np.float32)  # 1e3 standard deviations off in every column
    assert np.all(np.abs(x[7][None, :] - mu) >= 900 * np.sqrt(var))
    tab, cst = R.table(w, mu, var)
    e = R.estep(x, tab, cst)
    ll, labels, post, _ = run(gmm, x, tab, cst)
    ll, post = ll.cpu().numpy().astype(np.float64), post.cpu().numpy().astype(np.float64)
    assert np.isfinite(ll[7]) and ll[7] < -1e6 and abs(ll[7] - e["loglik"][7]) <= e["B_ll"][7]
    assert abs(post[7].sum() - 1.0) <= (K + 16) * U + 2 * e["Emax"][7]
    assert np.all(np.abs(ll - e["loglik"]) <= e["B_ll"])


def test_a_nan_row_changes_no_other_row(gmm):
    x, tab, cst, _ = ll_case(257, 65, 32)
    clean = x.copy()
    clean[37] = 0.0
    bad = clean.copy()
    bad[37, 5] = np.nan
    a, b = run(gmm, clean, tab, cst), run(gmm, bad, tab, cst)
    ll_a, ll_b = a[0].cpu().numpy(), b[0].cpu().numpy()
    assert np.isnan(ll_b[37]) and int(b[1][37]) == 0 and np.isfinite(ll_a).all()
    others = np.arange(257) != 37
    assert np.array_equal(bits(ll_a[others]), bits(ll_b[others])) and torch.equal(a[1][others], b[1][others])
    assert np.array_equal(bits(a[2].cpu().numpy()[others]), bits(b[2].cpu().numpy()[others]))


# -------------------------------------------------------------------------------------------------------------- statistics
def stats_np(s, D=None):
    return tuple(s[k].cpu().numpy()[..., :D] if k != "nk" else s[k].cpu().numpy() for k in ("nk", "sx", "sxx"))


@functools.lru_cache(maxsize=None)
def stats_case(N, K, D):
    x, w, mu, var = R.case(N, K, D)
    return (x,) + R.table(w, mu, var)


@pytest.mark.parametrize("D", [32, 39])
@pytest.mark.parametrize("N", STATS_N)
def test_statistics_against_the_float64_sums_of_the_devices_posteriors(gmm, N, D):
    for K in STATS_K:
        x, tab, cst = stats_case(N, K, D)
        xd = dev_rows(x)
        ll, _, post, _ = run(gmm, x, tab, cst)
        first = gmm.accumulate(xd, post)
        Dp = gmm.padded(D)
        assert tuple(first["sx"].shape) == (K, Dp) and first["nk"].dtype == torch.float64
        got = stats_np(first)
        assert not got[1][:, D:].any() and not got[2][:, D:].any()
        nk, sx, sxx, mags = R.stats(x, post.cpu().numpy())
        for name, g, want, mag in zip(("nk", "sx", "sxx"), (got[0], got[1][:, :D], got[2][:, :D]), (nk, sx, sxx), mags):
            s = share("stats " + name, np.abs(g - want), R.stats_bound(mag))
            assert s <= 1.0, (N, K, D, name, s)
        again = stats_np(gmm.accumulate(xd, post))
        for a, b in zip(got, again):
            assert np.array_equal(bits(a), bits(b)), (N, K, D)
        if N > R.SLICE:  # two row chunks cut at a slice boundary, the second onto the first
            cut = (N // R.SLICE) * R.SLICE if N % R.SLICE else N - R.SLICE
            two = gmm.accumulate(xd[:cut], post[:cut])
            two = gmm.accumulate(xd[cut:], post[cut:], two)
            for a, b in zip(got, stats_np(two)):
                assert np.array_equal(bits(a), bits(b)), (N, K, D, cut)


def test_estep_equals_the_raw_calls_over_its_chunks(gmm):
    N, K, D = 2500, 17, 39
    x, w, mu, var = R.case(N, K, D)
    model = {"weights": w, "means": mu, "variances": var}
    xd = dev_rows(x)
    S, ldp, Dp = gmm.GMM_SLICE, (K + 3) // 4 * 4, gmm.padded(D)
    max_bytes = S * ldp * 4 + gmm.ws_bytes(S, K, Dp)
    assert gmm.chunk_rows(N, K, D, max_bytes) == [S, S, N - 2 * S]
    stats, total, labels = gmm.estep(xd, model, max_bytes=max_bytes)
    assert tuple(stats["sx"].shape) == (K, D) and total.dtype == torch.float64 and labels.dtype == torch.int32
    tab, cst = gmm.table(model)
    want, want_total, want_labels, a = None, torch.zeros((), dtype=torch.float64, device="cuda"), [], 0
    for c in (S, S, N - 2 * S):
        ll, lab = gmm.loglik(xd[a:a + c], tab, cst)
        post = gmm.posteriors(xd[a:a + c], tab, cst, ll)
        want = gmm.accumulate(xd[a:a + c], post, want)
        want_total = want_total + ll.double().sum()
        want_labels.append(lab)
        a += c
    for g, w_ in zip(stats_np(stats), stats_np(want, D)):
        assert np.array_equal(bits(g), bits(w_))
    assert total.item() == want_total.item() and torch.equal(labels, torch.cat(want_labels))
    # one chunk: the same statistics bit for bit (the cuts are slice boundaries), and the oracle's E-step within the bounds
    whole, total_1, labels_1 = gmm.estep(xd, model)
    for g, w_ in zip(stats_np(stats), stats_np(whole)):
        assert np.array_equal(bits(g), bits(w_))
    assert torch.equal(labels, labels_1)
    e = R.estep(x, *R.table(w, mu, var))
    assert abs(total.item() - e["loglik"].sum()) <= e["B_ll"].sum() * 1.001 + 1e-3


# --------------------------------------------------------------------------------------------------------------------- fit
@functools.lru_cache(maxsize=None)
def blobs():
    rng = np.random.default_rng(61)
    centres = 12.0 * np.eye(6, 16) + 3.0 * rng.standard_normal((6, 16))
    x = np.concatenate([centres[b] + rng.standard_normal((500, 16)) for b in range(6)]).astype(np.float32)
    return x, np.repeat(np.arange(6), 500)


def test_fit_on_blobs(gmm):
    import units

    x, truth = blobs()
    assert sorted(truth[units.initial_rows(3000, 6, FIT_SEED)].tolist()) == list(range(6))  # the k-means start: one row per blob
    xd = dev_rows(x)
    model, hist = gmm.fit(xd, 6, iters=15, tol=0.0, seed=FIT_SEED)
    assert set(model) == {"weights", "means", "variances"} and all(v.dtype == torch.float64 and v.is_cuda for v in model.values())
    assert set(hist) == {"mean_loglik", "iterations", "converged", "starved", "floored"}
    assert hist["starved"] == 0 and 1 <= hist["iterations"] == len(hist["mean_loglik"]) <= 15
    w, mu, var = (model[k].cpu().numpy() for k in ("weights", "means", "variances"))
    sample = x.astype(np.float64).reshape(6, 500, 16).mean(axis=1)
    owner = np.abs(mu[:, None, :] - sample[None, :, :]).max(axis=2).argmin(axis=1)
    assert sorted(owner.tolist()) == list(range(6))
    nk = w * 3000
    assert np.all(np.abs(mu - sample[owner]) <= 4.0 / np.sqrt(nk)[:, None]) and np.all(np.abs(w - 1.0 / 6.0) <= 0.02)
    assert abs(w.sum() - 1.0) < 1e-6 and np.all(np.abs(var - 1.0) < 0.3)
    e = R.estep(x, *R.table(w, mu, var))
    slack = float(e["B_ll"].mean())
    assert all(b >= a - slack for a, b in zip(hist["mean_loglik"][:-1], hist["mean_loglik"][1:])), hist["mean_loglik"]
    again, hist2 = gmm.fit(xd, 6, iters=15, tol=0.0, seed=FIT_SEED)
    assert hist2 == hist
    for k in model:
        assert torch.equal(model[k].view(torch.int64), again[k].view(torch.int64))
    # the default stop rule ends it early, at a model the last entry of the history belongs to
    short, hist3 = gmm.fit(xd, 6, seed=FIT_SEED)
    assert hist3["converged"] and hist3["iterations"] < 15 and hist3["mean_loglik"] == hist["mean_loglik"][:hist3["iterations"]]
    stats, total, _ = gmm.estep(xd, short)
    assert total.item() / 3000 == hist3["mean_loglik"][-1]
    with pytest.raises(ValueError):
        gmm.fit(xd[:4], 5)


# --------------------------------------------------------------------------------------------------------------------- CLI
def feats_corpus(tmp_path, width=13):
    rs = np.random.RandomState(7)
    centres = 4.0 * rs.randn(4, width)
    keys, lens, items = [], [], []
    with open(tmp_path / "feats.scp", "w") as fs, open(tmp_path / "len.scp", "w") as ls:
        for u in range(5):
            key, n = "utt%02d" % u, 50 + 11 * u
            which = (np.arange(n) // 10 + u) % 4
            np.save(tmp_path / (key + ".npy"), (centres[which] + rs.randn(n, width)).astype(np.float32))
            fs.write("%s %s\n" % (key, tmp_path / (key + ".npy")))
            ls.write("%s %d\n" % (key, n))
            keys.append(key), lens.append(n)
            for k in range(4):
                items.append((key, 0.10 * k, 0.10 * k + 0.09, "p%d" % ((k + u) % 4), "b", "k", "s01"))
    import abx

    abx.write_items(str(tmp_path / "t.item"), items)
    return ["--feat-scp", str(tmp_path / "feats.scp"), "--len-scp", str(tmp_path / "len.scp")], keys, lens


GMM_KEYS = {"on", "k", "width", "frames", "iterations", "converged", "mean_loglik", "starved", "floored", "seed"}
ITEM_KEYS = {"cluster_purity", "phone_purity", "pnmi", "labelled_frames", "overlaps", "phones", "bitrate", "bitrate_collapsed"}


def test_fit_gmm_cli_without_a_checkpoint(gmm, tmp_path):
    import fit_gmm as FG
    import kaldi_io_lite as KIO
    import units

    base, keys, lens = feats_corpus(tmp_path)
    out, post_dir = tmp_path / "fit", tmp_path / "post"
    assert FG.main(base + ["--out", str(out), "--k", "4", "--on", "feats", "--post-out", str(post_dir)]) == 0
    assert sorted(p.name for p in out.iterdir()) == ["gmm.json", "gmm.npz", "units.txt", "units_collapsed.txt"]
    assert sorted(p.name for p in post_dir.iterdir()) == ["feats.ark", "feats.scp", "len.scp"]
    info = json.load(open(out / "gmm.json"))
    assert set(info) == GMM_KEYS
    assert info["on"] == "feats" and info["k"] == 4 and info["width"] == 13 and info["frames"] == sum(lens) and info["seed"] == 0
    assert info["iterations"] == len(info["mean_loglik"]) >= 1 and 0 <= info["starved"] < 4 and info["floored"] >= 0
    model = gmm.load(str(out / "gmm.npz"))
    # (the weights are the f32 posteriors' column sums over N: a row's posteriors sum to 1 within (K + 16) u + 2 max E)
    assert model["means"].shape == (4, 13) and abs(model["weights"].sum() - 1.0) < 1e-4
    # the archive: the posteriorgram of the rows bit for bit, every utterance in order, the input's len.scp
    rows = np.concatenate([np.load(tmp_path / (k + ".npy")) for k in keys])
    want, want_labels, _ = gmm.posteriorgram(to_dev(rows), model, with_labels=True)
    want, want_labels = want.cpu().numpy(), want_labels.cpu().numpy()
    assert want.shape == (sum(lens), 4) and np.allclose(want.sum(axis=1), 1.0, atol=1e-4)
    got = list(KIO.read_ark(str(post_dir / "feats.ark")))
    assert [k for k, _ in got] == keys and [len(m) for _, m in got] == lens
    assert np.array_equal(bits(np.concatenate([np.asarray(m, dtype=np.float32) for _, m in got])), bits(want))
    assert (post_dir / "len.scp").read_text() == (tmp_path / "len.scp").read_text()
    assert [line.split()[0] for line in (post_dir / "feats.scp").read_text().splitlines()] == keys
    got_keys, seqs = units.read_units(str(out / "units.txt"))
    assert got_keys == keys and np.array_equal(np.concatenate(seqs), want_labels)
    assert np.array_equal(want[np.arange(sum(lens)), want_labels], want.max(axis=1))
    _, collapsed = units.read_units(str(out / "units_collapsed.txt"))
    assert all(c.tolist() == units.collapse(s).tolist() for c, s in zip(collapsed, seqs))
    # --model with the written mixture: the same units and the same archive byte for byte; --item adds the quality keys
    again, post_again = tmp_path / "apply", tmp_path / "post_again"
    assert FG.main(base + ["--out", str(again), "--model", str(out / "gmm.npz"), "--on", "feats", "--post-out", str(post_again),
                           "--item", str(tmp_path / "t.item")]) == 0
    assert (again / "units.txt").read_bytes() == (out / "units.txt").read_bytes()
    assert (post_again / "feats.ark").read_bytes() == (post_dir / "feats.ark").read_bytes()
    same = gmm.load(str(again / "gmm.npz"))
    assert all(np.array_equal(bits(same[k]), bits(model[k])) for k in model)
    applied = json.load(open(again / "gmm.json"))
    assert set(applied) == GMM_KEYS | ITEM_KEYS and applied["iterations"] == 0 and applied["mean_loglik"] == [] and applied["converged"]
    assert 0.0 < applied["cluster_purity"] <= 1.0 and 0.0 < applied["phone_purity"] <= 1.0 and 0.0 <= applied["pnmi"] <= 1.0
    assert applied["phones"] == ["p0", "p1", "p2", "p3"] and applied["bitrate"] == pytest.approx(units.bitrate(seqs, 0.010)["bitrate"])
    # a model of another width, and more than 64 values per frame, are errors
    np.savez(str(tmp_path / "narrow.npz"), weights=np.ones(2) / 2, means=np.zeros((2, 12)), variances=np.ones((2, 12)))
    assert FG.main(base + ["--out", str(tmp_path / "no"), "--model", str(tmp_path / "narrow.npz"), "--on", "feats"]) == 1


def test_posteriorgrams_through_eval_model(gmm, tmp_path):
    import eval_model as EM
    import fit_gmm as FG

    base, keys, lens = tiny_corpus(tmp_path)
    item = str(tmp_path / "t.item")
    assert FG.main(base + ["--out", str(tmp_path / "gmm"), "--k", "4", "--on", "z1", "--post-out", str(tmp_path / "post")]) == 0
    assert json.load(open(tmp_path / "gmm" / "gmm.json"))["width"] == 16
    common = base + ["--max-recon", "2", "--abx-item", item]
    plain, with_b = tmp_path / "plain", tmp_path / "with"
    assert EM.main(common + ["--out", str(plain)]) == 0
    assert EM.main(common + ["--out", str(with_b), "--baseline-feat-scp", str(tmp_path / "post" / "feats.scp"), "--baseline-name", "gmm"]) == 0
    s_plain, s_with = json.load(open(plain / "summary.json")), json.load(open(with_b / "summary.json"))
    assert sorted(set(p.name for p in with_b.iterdir()) - set(p.name for p in plain.iterdir())) == ["abx_by_pair_gmm.tsv"]
    assert set(s_with) == set(s_plain) and set(s_with["abx"]) == set(s_plain["abx"]) | {"gmm"}
    for k in s_plain["abx"]:
        assert s_with["abx"][k] == s_plain["abx"][k], k
    assert all(s_with[k] == s_plain[k] for k in ("checkpoint", "segments", "sequences"))
    assert s_with["lower_bound_per_frame"] == pytest.approx(s_plain["lower_bound_per_frame"], rel=1e-6)  # (as tests/test_units_gpu.py)
    entry = s_with["abx"]["gmm"]
    assert set(entry) == set(s_plain["abx"]["z1"]) and entry["triples_within"] == s_plain["abx"]["z1"]["triples_within"]


def test_report_the_worst_share_of_each_bound(gmm):
    """(no assertion of its own: the shares asserted above, for the record of DESIGN §25)"""
    print("\nworst observed share of each bound:", json.dumps(WORST, sort_keys=True))
