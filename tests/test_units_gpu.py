"""Units on the GPU: fhvae_km_assign against the float64 scores of tests/kmeans_ref.py under the bound that follows from its
arithmetic, its tie rule and its row independence (bitwise); fhvae_km_update against the oracle's two-level float64 sums
(bitwise) and its status word; units.fit on blobs, against the float64 Lloyd oracle, on forced empty clusters and run twice;
discover_units.py and eval_model.py --units."""
import functools
import json

import numpy as np
import pytest
import torch

import kmeans_ref as R

pytestmark = pytest.mark.gpu

ASSIGN_N = (1, 63, 64, 255, 256, 257, 700)
ASSIGN_K = (1, 2, 15, 16, 17, 63, 64, 65, 130)
WIDE_N, WIDE_K = (63, 257, 700), (1, 17, 65, 130)
#: (N, K, D) -> seed where seed 0 leaves a row of a small case within 2 E of a tie (found with the oracle alone, on the CPU)
SEEDS = {(63, 130, 80): 1}
LLOYD_SEED, EMPTY_SEED = 0, 0


@pytest.fixture(scope="module")
def units():
    import build_ext

    build_ext.build(verbose=False)
    import units

    assert torch.cuda.is_available()
    units.load_library()
    return units


def dev_rows(a, pad=4, lead=0, extra_rows=0):
    """a (n, D) numpy -> the same values on the device as a view of a wider (and longer) allocation: leading dimension
    D + lead + pad, first column `lead` (a multiple of 4, so the rows stay 16-byte aligned)."""
    n, D = a.shape
    buf = torch.full((n + extra_rows, D + lead + pad), 77.0, dtype=torch.float32, device="cuda")
    view = buf[:n, lead:lead + D]
    view.copy_(torch.from_numpy(a))
    return view


@functools.lru_cache(maxsize=None)
def assign_case(N, K, D):
    """x, cent ~ N(0, 1) and what the oracle says of them, computed once."""
    rng = np.random.default_rng(1000003 * N + 1009 * K + D + 7919 * SEEDS.get((N, K, D), 0))
    x, cent = rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal((K, D)).astype(np.float32)
    s64, xn = R.scores(x, cent)
    labels, d64, gap, E = R.assign(x, cent)
    return x, cent, s64, labels, d64, gap, E


def check_assign(units, N, K, D):
    x, cent, s64, want, d64, gap, E = assign_case(N, K, D)
    near = gap <= 2 * E
    assert near.sum() <= 0.01 * N, "the case itself: %d of %d rows lie within 2 E of a tie" % (near.sum(), N)
    labels, dist = units.assign(dev_rows(x), dev_rows(cent, pad=4, lead=4))
    labels, dist = labels.cpu().numpy(), dist.cpu().numpy().astype(np.float64)
    assert labels.dtype == np.int32 and labels.min() >= 0 and labels.max() < K
    got = s64[np.arange(N), labels]
    assert np.all(got <= s64.min(axis=1) + 2 * E), (N, K, D)
    assert np.array_equal(labels[~near], want[~near]), (N, K, D)
    assert np.all(np.abs(dist - d64) <= 2 * E), (N, K, D, float(np.max(np.abs(dist - d64) / E)))
    only, none = units.assign(dev_rows(x), dev_rows(cent, pad=4, lead=4), want_dist=False)
    assert none is None and np.array_equal(only.cpu().numpy(), labels)


# ------------------------------------------------------------------------------------------------------------------ assign
@pytest.mark.parametrize("N", ASSIGN_N)
def test_assign_against_the_float64_scores(units, N):
    for K in ASSIGN_K:
        check_assign(units, N, K, 32)


@pytest.mark.parametrize("D", [16, 80, 128])
def test_assign_at_other_widths(units, D):
    for N in WIDE_N:
        for K in WIDE_K:
            check_assign(units, N, K, D)


@pytest.mark.parametrize("source, copies", [(5, (6, 12, 40, 100)), (127, (125, 115, 70, 9))])
def test_equal_centroids_go_to_the_smallest_index(units, source, copies):
    """copies of one centroid in the same group of four rows, in the same block of 16, in another block and in another tile of 64:
    bitwise equal scores, so the rows nearest to it get the smallest of the five indices"""
    rng = np.random.default_rng(11)
    K, D, N = 130, 32, 300
    cent = rng.standard_normal((K, D)).astype(np.float32)
    for c in copies:
        cent[c] = cent[source]
    x = rng.standard_normal((N, D)).astype(np.float32)
    mine = rng.permutation(N)[:60]
    x[mine] = cent[source] + 0.01 * rng.standard_normal((60, D)).astype(np.float32)
    five = sorted((source,) + tuple(copies))
    assert source // 4 == copies[0] // 4 and source // 16 == copies[1] // 16 != copies[2] // 16 and source // 64 != copies[3] // 64
    labels, dist = units.assign(dev_rows(x), dev_rows(cent))
    labels = labels.cpu().numpy()
    assert np.all(labels[mine] == five[0])
    assert not np.isin(labels, five[1:]).any()
    # a table whose every row is the same: every score of a row is equal, label 0
    same = np.repeat(cent[source][None, :], K, axis=0)
    assert not units.assign(dev_rows(x), dev_rows(same))[0].any()


def test_a_row_does_not_depend_on_its_batch(units):
    rng = np.random.default_rng(12)
    x, cent = rng.standard_normal((700, 32)).astype(np.float32), rng.standard_normal((65, 32)).astype(np.float32)
    xd, cd = dev_rows(x), dev_rows(cent)
    whole = units.assign(xd, cd)
    alone = units.assign(xd[100:400], cd)
    copy = units.assign(dev_rows(x[100:400], pad=12), cd)
    for part in (alone, copy):
        assert torch.equal(part[0], whole[0][100:400]) and torch.equal(part[1].view(torch.int32), whole[1][100:400].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ update
SIZES = (0, 1, 255, 256, 257, 1000)


@functools.lru_cache(maxsize=None)
def update_case(D):
    rng = np.random.default_rng(100 + D)
    N = sum(SIZES)
    labels = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int32)
    labels = labels[rng.permutation(N)]
    x = (rng.standard_normal((N, D)) * np.exp(3 * rng.standard_normal((N, 1)))).astype(np.float32)
    dist = rng.random(N).astype(np.float32) * 10
    cent = rng.standard_normal((len(SIZES), D)).astype(np.float32)
    return x, labels, dist, cent, R.update(x, labels, cent, dist)


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a.view(np.int64)


@pytest.mark.parametrize("D", [16, 32, 80, 128])
def test_update_equals_the_oracle_bit_for_bit(units, D):
    x, labels, dist, cent, (want_c, want_n, want_i) = update_case(D)
    assert want_n.tolist() == list(SIZES)
    xd, ld, dd = dev_rows(x, extra_rows=8), torch.from_numpy(labels).cuda(), torch.from_numpy(dist).cuda()
    runs = []
    for _ in range(2):
        cd = dev_rows(cent, pad=4, lead=4)
        count, inertia = units.update(xd, ld, cd, dd)
        runs.append((cd.cpu().numpy(), count.cpu().numpy(), inertia.cpu().numpy()))
    got_c, got_n, got_i = runs[0]
    assert got_n.dtype == np.int64 and np.array_equal(got_n, want_n)
    assert np.array_equal(bits(got_c), bits(want_c))
    assert np.array_equal(bits(got_i), bits(want_i)) and got_i[0] == 0.0
    assert np.array_equal(bits(got_c[0]), bits(cent[0]))  # the empty cluster keeps its row
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(bits(a), bits(b))
    # without dist: the same centroids, no inertia
    cd = dev_rows(cent)
    count, inertia = units.update(xd, ld, cd)
    assert np.array_equal(bits(cd.cpu().numpy()), bits(want_c)) and not inertia.any()


def test_update_of_one_cluster(units):
    rng = np.random.default_rng(5)
    x, dist = rng.standard_normal((300, 32)).astype(np.float32), rng.random(300).astype(np.float32)
    labels, cent = np.zeros(300, dtype=np.int32), np.zeros((1, 32), dtype=np.float32)
    want_c, want_n, want_i = R.update(x, labels, cent, dist)
    cd = dev_rows(cent)
    count, inertia = units.update(dev_rows(x), torch.from_numpy(labels).cuda(), cd, torch.from_numpy(dist).cuda())
    assert count.tolist() == [300] and np.array_equal(bits(cd.cpu().numpy()), bits(want_c))
    assert np.array_equal(bits(inertia.cpu().numpy()), bits(want_i))


def test_update_status_word(units):
    x, labels, dist, cent, _ = update_case(32)
    N, K = x.shape[0], cent.shape[0]
    xd = dev_rows(x, extra_rows=8)  # (a perm entry of N names allocated memory whatever the kernels do with it)
    ld = torch.from_numpy(labels).cuda()
    perm, cl_ptr = units.members(ld, K)
    assert cl_ptr.cpu().tolist() == np.concatenate([[0], np.cumsum(SIZES)]).tolist() and perm.dtype == torch.int64
    for bit, spoil in ((units.KM_BAD_PTR, "ptr"), (units.KM_BAD_PERM, "perm")):
        p, c = perm.clone(), cl_ptr.clone()
        if spoil == "ptr":
            c[3], c[4] = cl_ptr[4], cl_ptr[3]  # it decreases
        else:
            p[7] = N
        cd = dev_rows(cent)
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        count, inertia = units.update_members(xd, p, c, cd, status, torch.from_numpy(dist).cuda())
        assert int(status.item()) == bit
        assert np.array_equal(bits(cd.cpu().numpy()), bits(cent)) and not count.any() and not inertia.any()
        with pytest.raises(RuntimeError, match="status %d" % bit):
            units.check_status(status)
    bad = ld.clone()
    bad[5] = K  # a label outside [0, K): cl_ptr ends short of N
    with pytest.raises(RuntimeError, match="status 1"):
        units.update(xd, bad, dev_rows(cent))


# --------------------------------------------------------------------------------------------------------------------- fit
def blobs():
    rng = np.random.default_rng(21)
    centres = 20.0 * np.eye(5, 16)
    x = np.concatenate([centres[b] + rng.standard_normal((400, 16)) for b in range(5)]).astype(np.float32)
    return x, np.repeat(np.arange(5), 400)


def test_fit_on_blobs(units):
    x, truth = blobs()
    xd = dev_rows(x)
    res = units.fit(xd, 5, init=x[::400][:5].copy())
    assert set(res) == {"centroids", "labels", "counts", "inertia", "iterations", "converged", "reseeded"}
    assert res["converged"] and res["iterations"] <= 3 and res["reseeded"] == 0
    assert np.array_equal(res["labels"].cpu().numpy(), truth) and res["counts"].tolist() == [400] * 5
    assert res["inertia"] == pytest.approx(float(((x - x.reshape(5, 400, 16).mean(axis=1).repeat(400, axis=0)) ** 2).sum()), rel=1e-4)
    # from rows drawn at random (blobs share centroids at first): the inertia never rises
    last = None
    for iters in range(1, 7):
        r = units.fit(xd, 5, iters=iters, tol=0.0, seed=3)
        if r["iterations"] < iters:
            break
        assert last is None or r["inertia"] <= last * (1 + 1e-6), iters
        last = r["inertia"]
    assert last is not None
    with pytest.raises(ValueError):
        units.fit(xd[:4], 5)
    bad = xd.clone()
    bad[17, 3] = float("nan")
    with pytest.raises(ValueError):
        units.fit(bad, 5)


@functools.lru_cache(maxsize=None)
def lloyd_case():
    rng = np.random.default_rng(31 + LLOYD_SEED)
    x = rng.standard_normal((600, 16)).astype(np.float32)
    import units as U

    init = x[U.initial_rows(600, 8, 4)]
    return x, init, R.lloyd(x, init, 5, tol=0.0)


def test_fit_follows_the_float64_lloyd_oracle(units):
    x, init, hist = lloyd_case()
    assert len(hist) == 5 and all(h["min_margin"] > 0 and not h["reseeded"] for h in hist)  # no row within 2 E of a tie
    xd = dev_rows(x)
    for it, h in enumerate(hist, 1):
        r = units.fit(xd, 8, iters=it, tol=0.0, seed=4)
        assert r["iterations"] == it
        assert np.array_equal(r["labels"].cpu().numpy(), h["labels"]), it
        assert np.array_equal(bits(r["centroids"].cpu().numpy()), bits(h["centroids"])), it  # (the update is exact, so they stay equal)
        assert np.array_equal(r["counts"], h["counts"]) and r["inertia"] == pytest.approx(h["inertia"], rel=1e-5)
    by_init = units.fit(xd, 8, iters=5, tol=0.0, init=init)
    assert np.array_equal(by_init["labels"].cpu().numpy(), hist[-1]["labels"])


def test_empty_clusters_take_the_farthest_rows(units):
    rng = np.random.default_rng(41 + EMPTY_SEED)
    x = rng.standard_normal((300, 16)).astype(np.float32)
    x[45] *= 4.0  # the farthest row from its centroid (d = 362), then row 123 (d = 247); the third lies at 40
    x[123] *= 5.0
    far = np.full(16, 10.0, np.float32)  # no row is nearer to +-far than to one of the three rows
    init = np.stack([x[0], far, x[1], -far, x[2]])
    first = R.assign(x, init)
    assert np.bincount(first[0], minlength=5)[[1, 3]].tolist() == [0, 0] and np.argsort(-first[1])[:2].tolist() == [45, 123]
    hist = R.lloyd(x, init, 1, tol=0.0)
    assert hist[0]["min_margin"] > 0 and hist[0]["reseeded"] and hist[0]["labels"][45] == 1 and hist[0]["labels"][123] == 3
    r = units.fit(dev_rows(x), 5, iters=1, init=init)
    labels = r["labels"].cpu().numpy()
    assert r["reseeded"] == 1 and np.array_equal(labels, hist[0]["labels"]) and r["counts"][1] == 1 and r["counts"][3] == 1
    cent = r["centroids"].cpu().numpy()
    assert np.array_equal(bits(cent), bits(hist[0]["centroids"])) and np.array_equal(bits(cent[1]), bits(x[45]))
    assert np.array_equal(bits(cent[3]), bits(x[123]))


def test_fit_twice_gives_the_same_bits(units):
    rng = np.random.default_rng(51)
    xd = dev_rows(rng.standard_normal((2000, 32)).astype(np.float32))
    a, b = (units.fit(xd, 20, iters=8, n_init=2, seed=9) for _ in range(2))
    assert torch.equal(a["labels"], b["labels"]) and torch.equal(a["centroids"].view(torch.int32), b["centroids"].view(torch.int32))
    assert a["inertia"] == b["inertia"] and a["iterations"] == b["iterations"] and np.array_equal(a["counts"], b["counts"])
    assert int(a["counts"].sum()) == 2000


# --------------------------------------------------------------------------------------------------------------------- CLI
def tiny_corpus(tmp_path):
    """T = 20, F = 16, H = 32, D = 16, six utterances of two speakers, an alignment of three phones (tests/test_abx_gpu.py)."""
    import abx
    import utils
    from fhvae import FHVAE

    T, F, H, D = 20, 16, 32, 16
    rs = np.random.RandomState(3)
    keys, lens, items = [], [], []
    phones = ["aa", "iy", "s"]
    with open(tmp_path / "feats.scp", "w") as fs, open(tmp_path / "len.scp", "w") as ls:
        for s in range(2):
            for u in range(3):
                key, n = "s%02d-1-%04d" % (s + 1, u), 60 + 7 * u
                np.save(tmp_path / (key + ".npy"), (rs.randn(n, F) + s).astype(np.float32))
                fs.write("%s %s\n" % (key, tmp_path / (key + ".npy")))
                ls.write("%s %d\n" % (key, n))
                keys.append(key), lens.append(n)
                for k in range(6):
                    items.append((key, 0.08 * k, 0.08 * k + 0.05, phones[(k + u) % 3], "b", "k", "s%02d" % (s + 1)))
    items.append(("nobody", 0.0, 0.1, "aa", "b", "k", "s01"))
    abx.write_items(str(tmp_path / "t.item"), items)
    torch.manual_seed(5)
    m = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, num_seqs=len(keys))
    utils.save_checkpoint(m, None, [], {}, "t", 1, 1, 0.0, 0.0, str(tmp_path))
    base = ["--checkpoint", str(tmp_path / "fhvae_t_e1.tar"), "--feat-scp", str(tmp_path / "feats.scp"), "--len-scp", str(tmp_path / "len.scp")]
    return base, keys, lens


FIT_KEYS = {"on", "k", "frames", "iterations", "converged", "inertia", "reseeded", "seed", "bitrate", "bitrate_collapsed"}
ITEM_KEYS = {"cluster_purity", "phone_purity", "pnmi", "labelled_frames", "overlaps", "phones"}


def test_discover_units_cli(units, tmp_path):
    import discover_units as DU

    base, keys, lens = tiny_corpus(tmp_path)
    for on in ("z1", "feats"):
        out, again = tmp_path / ("fit_" + on), tmp_path / ("apply_" + on)
        assert DU.main(base + ["--out", str(out), "--k", "4", "--on", on, "--item", str(tmp_path / "t.item")]) == 0
        assert sorted(p.name for p in out.iterdir()) == ["units.json", "units.txt", "units_centroids.npy", "units_collapsed.txt", "units_counts.npy"]
        got_keys, seqs = units.read_units(str(out / "units.txt"))
        assert got_keys == keys and [len(s) for s in seqs] == lens and all(0 <= s.min() and s.max() < 4 for s in seqs)
        _, collapsed = units.read_units(str(out / "units_collapsed.txt"))
        assert all(c.tolist() == units.collapse(s).tolist() for c, s in zip(collapsed, seqs))
        cent, counts = np.load(out / "units_centroids.npy"), np.load(out / "units_counts.npy")
        assert cent.shape == (4, 16) and cent.dtype == np.float32 and counts.dtype == np.int64
        assert counts.tolist() == np.bincount(np.concatenate(seqs), minlength=4).tolist()
        info = json.load(open(out / "units.json"))
        assert set(info) == FIT_KEYS | ITEM_KEYS
        assert info["on"] == on and info["k"] == 4 and info["frames"] == sum(lens) and info["seed"] == 0 and info["iterations"] >= 1
        assert info["phones"] == ["aa", "iy", "s"] and info["labelled_frames"] == 36 * 6 and info["overlaps"] == 0
        assert 0.0 < info["cluster_purity"] <= 1.0 and 0.0 < info["phone_purity"] <= 1.0 and 0.0 <= info["pnmi"] <= 1.0
        assert info["bitrate"] == pytest.approx(units.bitrate(seqs, 0.010)["bitrate"]) and 0 < info["bitrate_collapsed"] <= info["bitrate"]
        # the written codebook, applied: the same units byte for byte
        assert DU.main(base + ["--out", str(again), "--codebook", str(out / "units_centroids.npy"), "--on", on]) == 0
        assert (again / "units.txt").read_bytes() == (out / "units.txt").read_bytes()
        applied = json.load(open(again / "units.json"))
        assert set(applied) == FIT_KEYS and applied["iterations"] == 0 and applied["inertia"] == info["inertia"]
    np.save(tmp_path / "narrow.npy", np.zeros((4, 12), dtype=np.float32))
    assert DU.main(base + ["--out", str(tmp_path / "no"), "--codebook", str(tmp_path / "narrow.npy")]) == 1


def test_eval_model_cli_with_units(units, tmp_path):
    import eval_model as EM

    base, keys, lens = tiny_corpus(tmp_path)
    base = base + ["--max-recon", "2"]
    plain, with_units, only = tmp_path / "plain", tmp_path / "units", tmp_path / "only"
    assert EM.main(base + ["--out", str(plain)]) == 0
    assert EM.main(base + ["--out", str(with_units), "--units", "4", "--units-item", str(tmp_path / "t.item")]) == 0
    s_plain, s_units = json.load(open(plain / "summary.json")), json.load(open(with_units / "summary.json"))
    assert "units" not in s_plain
    names = sorted(p.name for p in with_units.iterdir())
    assert sorted(p.name for p in plain.iterdir()) == [n for n in names if not n.startswith("units_")]
    assert [n for n in names if n.startswith("units_")] == ["units_centroids_feats.npy", "units_centroids_z1.npy", "units_feats.txt", "units_z1.txt"]
    block = s_units.pop("units")
    assert set(s_units) == set(s_plain) and all(s_units[k] == s_plain[k] for k in ("checkpoint", "segments", "sequences"))
    assert s_units["lower_bound_per_frame"] == pytest.approx(s_plain["lower_bound_per_frame"], rel=1e-6)
    for name in sorted(p.name for p in plain.iterdir() if p.name.endswith(".npy")):
        assert np.load(plain / name).shape == np.load(with_units / name).shape, name
    assert set(block) == {"z1", "feats"}
    for on in ("z1", "feats"):
        assert set(block[on]) == FIT_KEYS | ITEM_KEYS and block[on]["on"] == on and block[on]["k"] == 4 and block[on]["frames"] == sum(lens)
        got_keys, seqs = units.read_units(str(with_units / ("units_%s.txt" % on)))
        assert got_keys == keys and [len(s) for s in seqs] == lens
        assert np.load(with_units / ("units_centroids_%s.npy" % on)).shape == (4, 16)
    assert EM.main(base + ["--out", str(only), "--units", "3", "--units-on", "feats", "--units-iters", "2", "--units-seed", "1"]) == 0
    block = json.load(open(only / "summary.json"))["units"]
    assert set(block) == {"feats"} and set(block["feats"]) == FIT_KEYS and block["feats"]["iterations"] <= 2 and block["feats"]["seed"] == 1
    assert not (only / "units_z1.txt").exists() and (only / "units_feats.txt").exists()
