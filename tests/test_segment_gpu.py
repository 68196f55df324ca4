"""Segmentation on the GPU: fhvae_seg_scores against the float64 cells of tests/segment_ref.py under the derived bound B, its
+inf / -1 cells, its arg-min outside the 2 B gap and its tie rule; fhvae_seg_dp against the oracle's recursion run on the
DOWNLOADED device scores and units, bit for bit (segments, units, counts, costs, ties); the end-to-end objective against the
float64 optimum; planted cases; batch, position and grouping independence (bitwise); and what the kernels refuse.

Observed on an MI355X: the worst |score - score64| / B over the sweep (printed by test_cells) is 0.090, at D = 16; 0.059 at
D = 32."""
import functools

import numpy as np
import pytest
import torch

import segment_cases as SC
import segment_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def seg():
    import build_ext

    build_ext.build(verbose=False)
    import segment

    assert torch.cuda.is_available()
    segment.load_library()
    return segment


def dev_rows(a, pad=0, stride=1):
    """a (n, D) numpy -> the same values on the device, as a view of an allocation with `pad` more columns (a leading dimension
    of D + pad) and of every `stride`-th row of it."""
    n, D = a.shape
    buf = torch.full((max(n, 1) * stride, D + pad), 77.0, dtype=torch.float32, device="cuda")
    view = buf[::stride][:n, :D]
    view.copy_(torch.tensor(np.ascontiguousarray(a)))
    return view


@functools.lru_cache(maxsize=None)
def run(name):
    """The case on the device, once: the downloaded scores and units, and fhvae_seg_dp's outputs for every lambda."""
    import segment

    c = SC.case(name)
    x = dev_rows(c["x"], pad=4 if c["pad_x"] else 0)
    cent = dev_rows(c["cent"], stride=2 if c["stride_c"] else 1)
    if c["pad_x"]:
        assert x.stride(0) == c["D"] + 4
    if c["stride_c"]:
        assert cent.stride(0) == 2 * c["D"]
    ptr = torch.tensor(c["ptr"]).cuda()
    score, unit = segment.scores(x, cent, ptr, c["L"])
    out = {"score": score.cpu().numpy(), "unit": unit.cpu().numpy(), "dp": {}}
    for lam in SC.LAMBDAS:
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        got = segment.dp(score, unit, ptr, lam, status=status)
        out["dp"][lam] = tuple(t.cpu().numpy() for t in got) + (int(status.item()),)
    return out


WORST = {}


@pytest.mark.parametrize("name", SC.NAMES)
def test_cells(seg, name):
    c, got = SC.case(name), run(name)
    score, unit = got["score"], got["unit"]
    assert score.dtype == np.float32 and unit.dtype == np.int32 and score.shape == unit.shape == (int(c["ptr"][-1]), c["L"])
    fin = np.isfinite(c["score"])
    # +inf / -1 exactly where the segment crosses the utterance's start
    assert np.array_equal(np.isposinf(score), ~fin) and np.array_equal(unit == -1, ~fin) and not np.isnan(score).any()
    for u in range(len(c["lengths"])):
        a, b = int(c["ptr"][u]), int(c["ptr"][u + 1])
        for n in range(a, min(b, a + c["L"])):
            assert fin[n].sum() == min(n - a + 1, c["L"]) and fin[n, :n - a + 1].all()
    # the bound on every finite cell
    diff = np.abs(score.astype(np.float64)[fin] - c["score"][fin])
    ratio = float((diff / c["B"][fin]).max()) if fin.any() else 0.0
    WORST[name] = ratio
    print("%s: worst |score - score64| / B = %.4f over %d cells (worst so far over the sweep: %.4f)" % (name, ratio, int(fin.sum()), max(WORST.values())))
    assert (diff <= c["B"][fin]).all()
    # the arg-min wherever the runner-up is clear of the best by more than 2 B; at most 1 % of the cells are not
    clear = fin & (c["gap"] > 2 * c["B"])
    assert SC.inside_gap(c) <= 0.01
    assert np.array_equal(unit[clear], c["unit"][clear])
    assert ((unit[fin] >= 0) & (unit[fin] < c["K"])).all()


def test_duplicate_centroid_rows_give_the_smaller_index(seg):
    rng = np.random.default_rng(31)
    x = rng.standard_normal((200, 32)).astype(np.float32)
    cent = rng.standard_normal((70, 32)).astype(np.float32)
    cent[5], cent[66], cent[69] = cent[3], cent[3], cent[40]  # (within a tile of 64 centroids and across two)
    x[20:60] = cent[3] + 0.1 * x[20:60]  # (rows for which the duplicated centroids are the best)
    x[130:160] = cent[40] + 0.1 * x[130:160]
    ptr = torch.tensor([0, 120, 200], device="cuda")
    score, unit = seg.scores(dev_rows(x), dev_rows(cent), ptr, 7)
    unit = unit.cpu().numpy()
    assert not np.isin(unit, (5, 66, 69)).any() and (unit == 3).any() and (unit == 40).any()
    want = R.batch_scores(x, cent, [0, 120, 200], 7)
    clear = np.isfinite(want[0]) & ((want[2] > 2 * want[3]) | np.isin(want[1], (3, 40)))
    assert np.array_equal(unit[clear], want[1][clear])


@pytest.mark.parametrize("name", SC.NAMES)
def test_dp_bit_for_bit_on_the_device_scores(seg, name):
    """The oracle's recursion on the DOWNLOADED scores and units: the same segments, units, counts, and the same cost bits."""
    c, got = SC.case(name), run(name)
    for lam in SC.LAMBDAS:
        seg_unit, seg_start, n_seg, cost, status = got["dp"][lam]
        assert status == 0 and seg_unit.dtype == np.int32 and seg_start.dtype == np.uint8 and cost.dtype == np.float64
        for u, T in enumerate(c["lengths"]):
            a, b = int(c["ptr"][u]), int(c["ptr"][u + 1])
            starts, units, want_cost, flag = R.dp(got["score"][a:b], got["unit"][a:b], lam)
            want_unit, want_start = R.frame_outputs(starts, units, int(T))
            assert flag == 0 and n_seg[u] == len(starts), (name, lam, u)
            assert np.array_equal(seg_start[a:b], want_start) and np.array_equal(seg_unit[a:b], want_unit), (name, lam, u)
            assert np.float64(cost[u]).tobytes() == np.float64(want_cost).tobytes(), (name, lam, u, cost[u], want_cost)
            if T == 0:
                assert n_seg[u] == 0 and cost[u] == 0.0


def test_dp_ties_take_the_smallest_length(seg):
    """Scores on which every sum is exact and ties abound (small integers, dyadic lambdas), fed to fhvae_seg_dp directly."""
    rng = np.random.default_rng(32)
    lengths = [1, 2, 3, 0, 7, 64, 65, 130, 2100]
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    for L in (1, 3, 64):
        score = rng.integers(-1, 2, size=(int(ptr[-1]), L)).astype(np.float32)
        unit = rng.integers(0, 9, size=score.shape).astype(np.int32)
        for a in ptr[:-1]:
            for n in range(int(a), min(int(a) + L, int(ptr[-1]))):
                score[n, n - int(a) + 1:] = np.inf
        zero = np.zeros_like(score)
        zero[np.isinf(score)] = np.inf
        for table in (score, zero):
            for lam in (0.0, 0.25, 4.0):
                seg_unit, seg_start, n_seg, cost = (t.cpu().numpy() for t in seg.dp(torch.tensor(table).cuda(), torch.tensor(unit).cuda(),
                                                                                    torch.tensor(ptr).cuda(), lam))
                for u, T in enumerate(lengths):
                    a, b = int(ptr[u]), int(ptr[u + 1])
                    starts, units, want_cost, _ = R.dp(table[a:b], unit[a:b], lam)
                    want_unit, want_start = R.frame_outputs(starts, units, T)
                    assert n_seg[u] == len(starts) and cost[u] == want_cost, (L, lam, u)
                    assert np.array_equal(seg_start[a:b], want_start) and np.array_equal(seg_unit[a:b], want_unit), (L, lam, u)
                    if table is zero and lam == 0.0:
                        assert n_seg[u] == T  # every cut costs 0: one frame per segment


@pytest.mark.parametrize("name", SC.NAMES)
def test_end_to_end_objective(seg, name):
    """J64(device segmentation) <= J64* + 2 (sum of B over the segments of both paths) + T 2^-52 max |alpha|: the DP is exact on
    the device's scores, so the slack is the scores' alone."""
    c, got = SC.case(name), run(name)
    for lam in SC.LAMBDAS:
        seg_unit, seg_start, n_seg, cost, status = got["dp"][lam]
        for u, T in enumerate(c["lengths"]):
            a, b = int(c["ptr"][u]), int(c["ptr"][u + 1])
            if T == 0:
                continue
            x = c["x"][a:b]
            dev_starts = np.nonzero(seg_start[a:b])[0]
            dev_units = seg_unit[a:b][dev_starts]
            alpha, _ = R.dp_alpha(c["score"][a:b], lam)
            ref_starts, ref_units, best, _ = R.dp(c["score"][a:b], c["unit"][a:b], lam)
            j_dev = R.objective(x, c["cent"], dev_starts, dev_units, lam)
            slack = 2 * (R.bound_of(c["B"][a:b], dev_starts, int(T)) + R.bound_of(c["B"][a:b], ref_starts, int(T))) + T * 2.0 ** -52 * np.abs(alpha).max()
            assert j_dev <= best + slack, (name, lam, u, j_dev, best, slack)
            assert j_dev >= best - T * 2.0 ** -50 * max(np.abs(alpha).max(), 1.0), (name, lam, u)  # (nothing beats the optimum)


def test_planted_cases(seg):
    """Runs of 1 .. Lmax frames of centroids at least 1 apart, noise 1e-3, lambda 0.1: the plant, exactly."""
    rng = np.random.default_rng(33)
    for K, D, L in ((2, 16, 1), (17, 32, 5), (65, 32, 32), (65, 32, 64)):
        x, cent, lengths, truth = R.planted(rng, 9, K, D, L)
        segs, costs = seg.segment(torch.tensor(x).cuda(), torch.tensor(cent).cuda(), lengths, 0.1, L)
        ptr = np.concatenate([[0], np.cumsum(lengths)])
        for u, ((starts, units), (want_starts, want_units)) in enumerate(zip(segs, truth)):
            o = R.scores(x[ptr[u]:ptr[u + 1]], cent, L)
            ref_starts, ref_units, best, _ = R.dp(o[0], o[1], 0.1)
            assert ref_starts.tolist() == want_starts.tolist() and ref_units.tolist() == want_units.tolist()
            assert starts.tolist() == want_starts.tolist() and units.tolist() == want_units.tolist(), (K, L, u)
            assert starts.dtype == np.int64 and units.dtype == np.int32
            assert abs(costs[u] - best) <= 2 * R.bound_of(o[3], ref_starts, int(lengths[u])) + 1e-12


def test_batch_and_grouping_independence(seg):
    """An utterance gives the same bits alone, in a batch (at another position of the workgroups' tiles), and when segment() is
    forced into several groups."""
    c, got = SC.case("mixed7"), run("mixed7")
    x, cent = torch.tensor(c["x"]).cuda(), torch.tensor(c["cent"]).cuda()
    for u, T in enumerate(c["lengths"]):
        a, b = int(c["ptr"][u]), int(c["ptr"][u + 1])
        if T == 0:
            continue
        ptr = torch.tensor([0, int(T)], device="cuda")
        score, unit = seg.scores(x[a:b], cent, ptr, c["L"])
        assert np.array_equal(score.cpu().numpy().view(np.uint32), got["score"][a:b].view(np.uint32))
        assert np.array_equal(unit.cpu().numpy(), got["unit"][a:b])
        for lam in SC.LAMBDAS:
            seg_unit, seg_start, n_seg, cost = (t.cpu().numpy() for t in seg.dp(score, unit, ptr, lam))
            want = got["dp"][lam]
            assert np.array_equal(seg_unit, want[0][a:b]) and np.array_equal(seg_start, want[1][a:b])
            assert n_seg[0] == want[2][u] and cost.tobytes() == want[3][u:u + 1].tobytes()
    # segment(): one group, and groups of a few utterances (the limit leaves room for about 350 frames beside the fixed part)
    fixed = 4 * c["K"] + 768 + min(int(c["ptr"][-1]), seg.SEG_CHUNK_ROWS) * c["L"] * c["D"] * 4
    whole = seg.segment(x, cent, c["lengths"], 0.25, c["L"])
    split = seg.segment(x, cent, c["lengths"], 0.25, c["L"], ws_limit=fixed + 350 * (8 * c["L"] + 17))
    tiny = seg.segment(x, cent, c["lengths"], 0.25, c["L"], ws_limit=1)
    seg_unit, seg_start, n_seg, cost, _ = got["dp"][0.25]
    for segs, costs in (whole, split, tiny):
        assert costs.tobytes() == cost.tobytes()
        for u, (starts, units) in enumerate(segs):
            a, b = int(c["ptr"][u]), int(c["ptr"][u + 1])
            assert starts.tolist() == np.nonzero(seg_start[a:b])[0].tolist() and units.tolist() == seg_unit[a:b][starts].tolist()
            assert len(starts) == n_seg[u]
    import hip_ext

    per = c["lengths"] * (8 * c["L"] + 17)
    assert len(hip_ext.groups(per, 350 * (8 * c["L"] + 17))) > 1 and len(hip_ext.groups(per, 1)) == len(c["lengths"])


def test_refusals(seg):
    c = SC.case("L5_K17")
    x, cent = torch.tensor(c["x"]).cuda(), torch.tensor(c["cent"]).cuda()
    N, L, U = int(c["ptr"][-1]), c["L"], len(c["lengths"])
    # a utt_ptr that is not monotone, one that does not end at the rows: FHVAE_SEG_BAD_PTR, and nothing is written
    for bad in (c["ptr"][[0, 2, 1] + list(range(3, U + 1))], np.concatenate([c["ptr"][:-1], [N - 1]]), np.concatenate([[1], c["ptr"][1:]])):
        ptr = torch.tensor(np.ascontiguousarray(bad)).cuda()
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = (torch.full((N, L), -7.0, device="cuda"), torch.full((N, L), -7, dtype=torch.int32, device="cuda"))
        seg.scores(x, cent, ptr, L, status=status, out=out)
        assert int(status.item()) == seg.SEG_BAD_PTR and bool((out[0] == -7.0).all()) and bool((out[1] == -7).all())
        with pytest.raises(RuntimeError, match="utt_ptr"):
            seg.scores(x, cent, ptr, L)
        status.zero_()
        good = run("L5_K17")
        outs = (torch.full((N,), -7, dtype=torch.int32, device="cuda"), torch.full((N,), 7, dtype=torch.uint8, device="cuda"),
                torch.full((U,), -7, dtype=torch.int32, device="cuda"), torch.full((U,), -7.0, dtype=torch.float64, device="cuda"))
        seg.dp(torch.tensor(good["score"]).cuda(), torch.tensor(good["unit"]).cuda(), ptr, 0.25, status=status, out=outs)
        assert int(status.item()) == seg.SEG_BAD_PTR
        assert all(bool((t == (7 if t.dtype == torch.uint8 else -7)).all()) for t in outs)
    # a NaN row: the not-finite bit, for that utterance only
    bad_u = 7  # (T = 64)
    rows = c["x"].copy()
    rows[int(c["ptr"][bad_u]) + 10, 3] = np.nan
    ptr = torch.tensor(c["ptr"]).cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    score, unit = seg.scores(torch.tensor(rows).cuda(), cent, ptr, L, status=status)
    seg_unit, seg_start, n_seg, cost = (t.cpu().numpy() for t in seg.dp(score, unit, ptr, 0.25, status=status))
    assert int(status.item()) == seg.SEG_NOT_FINITE
    want = run("L5_K17")["dp"][0.25]
    a, b = int(c["ptr"][bad_u]), int(c["ptr"][bad_u + 1])
    assert n_seg[bad_u] == -1 and cost[bad_u] == np.inf and (seg_unit[a:b] == -1).all() and (seg_start[a:b] == 0).all()
    keep = np.ones(N, dtype=bool)
    keep[a:b] = False
    others = np.arange(U) != bad_u
    assert np.array_equal(seg_unit[keep], want[0][keep]) and np.array_equal(seg_start[keep], want[1][keep])
    assert np.array_equal(n_seg[others], want[2][others]) and cost[others].tobytes() == want[3][others].tobytes()
    with pytest.raises(RuntimeError, match="finite"):
        seg.segment(torch.tensor(rows).cuda(), cent, c["lengths"], 0.25, L)


# --------------------------------------------------------------------------------------------------------------------- CLI
def tiny_corpus(tmp_path):
    """T = 20, F = 16, H = 32, D = 16, six utterances of two speakers, an alignment of three phones (tests/test_units_gpu.py)."""
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
                    items.append((key, 0.08 * k, 0.08 * k + 0.07, phones[(k + u) % 3], "b", "k", "s%02d" % (s + 1)))
    abx.write_items(str(tmp_path / "t.item"), items)
    torch.manual_seed(5)
    m = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, num_seqs=len(keys))
    utils.save_checkpoint(m, None, [], {}, "t", 1, 1, 0.0, 0.0, str(tmp_path))
    base = ["--checkpoint", str(tmp_path / "fhvae_t_e1.tar"), "--feat-scp", str(tmp_path / "feats.scp"), "--len-scp", str(tmp_path / "len.scp")]
    return base, keys, lens


def test_discover_units_cli_with_segment(seg, tmp_path):
    import json

    import abx
    import discover_units as DU
    import units

    base, keys, lens = tiny_corpus(tmp_path)
    plain, out = tmp_path / "plain", tmp_path / "seg"
    common = ["--k", "4", "--on", "feats", "--item", str(tmp_path / "t.item")]
    assert DU.main(base + common + ["--out", str(plain)]) == 0
    assert DU.main(base + common + ["--out", str(out), "--segment", "--dur-penalty", "8", "--max-seg-frames", "12"]) == 0
    old = sorted(p.name for p in plain.iterdir())
    assert sorted(p.name for p in out.iterdir()) == sorted(old + ["segments.item", "segments.txt"])
    for name in old:
        if name != "units.json":
            assert (plain / name).read_bytes() == (out / name).read_bytes(), name
    info = json.load(open(out / "units.json"))
    block = info.pop("segments")
    assert json.dumps(info, indent=1) == (plain / "units.json").read_text()
    got_keys, seqs = units.read_units(str(out / "segments.txt"))
    assert got_keys == keys and sum(len(s) for s in seqs) == block["segments"] and all(0 <= s.min() and s.max() < 4 for s in seqs)
    assert block["dur_penalty"] == 8.0 and block["max_seg_frames"] == 12 and block["mean_frames"] == sum(lens) / block["segments"]
    assert all(-(-n // 12) <= len(s) <= n for s, n in zip(seqs, lens))
    assert block["bitrate_segments"] == pytest.approx(units._bits(seqs, sum(lens) * 0.010)) and block["bitrate_segments"] <= info["bitrate"]
    for key in ("precision", "recall", "f", "os", "r_value", "hits", "hyp_boundaries", "ref_boundaries", "utterances", "cluster_purity",
                "phone_purity", "pnmi", "labelled_frames"):
        assert key in block, key
    assert block["utterances"] == 6 and block["ref_boundaries"] == 6 * 5 and block["hyp_boundaries"] == block["segments"] - 6
    its = abx.read_items(str(out / "segments.item"))
    assert len(its) == block["segments"] and [it[0] for it in its] == [k for k, s in zip(keys, seqs) for _ in s]
    assert [it[3] for it in its] == ["u%d" % u for s in seqs for u in s]
    # the items tile every utterance: the segments' frames, one after the other
    at = {}
    for it in its:
        first, count = abx.frame_range(it[1], it[2], lens[keys.index(it[0])])
        assert first == at.get(it[0], 0) and 1 <= count <= 12
        at[it[0]] = first + count
    assert [at[k] for k in keys] == lens


def test_eval_model_cli_with_units_segment(seg, tmp_path):
    import json

    import eval_model as EM

    base, keys, lens = tiny_corpus(tmp_path)
    base = base + ["--max-recon", "2", "--units", "4", "--units-on", "feats"]
    plain, out = tmp_path / "plain", tmp_path / "seg"
    assert EM.main(base + ["--out", str(plain)]) == 0
    assert EM.main(base + ["--out", str(out), "--units-segment", "--units-dur-penalty", "8", "--units-max-seg-frames", "12"]) == 0
    old = sorted(p.name for p in plain.iterdir())
    assert sorted(p.name for p in out.iterdir()) == sorted(old + ["segments_feats.item", "segments_feats.txt"])
    a, b = json.load(open(plain / "summary.json")), json.load(open(out / "summary.json"))
    block = b["units"]["feats"].pop("segments")
    assert a["units"] == b["units"] and block["max_seg_frames"] == 12 and block["segments"] >= sum(-(-n // 12) for n in lens)
    assert (plain / "units_feats.txt").read_bytes() == (out / "units_feats.txt").read_bytes()
