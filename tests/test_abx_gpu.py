"""ABX on the GPU: fhvae_abx_dtw against the scalar oracle (tests/abx_ref.py), its structure (symmetry, the diagonal, batch and
order invariance, overlapping tokens), its status word, abx.pair_distances + abx_scores on planted data against the literal
triple loop, and eval_model.py --abx-item."""
import functools
import json

import numpy as np
import pytest
import torch

import abx_ref as R

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 17, 63, 64)
#: (D, metric) -> seed, chosen on the CPU so that the oracle's smallest on-path gap of every pair is at least MIN_GAP
SEEDS = {(3, "angular"): 0, (3, "cosine"): 0, (32, "angular"): 0, (32, "cosine"): 0, (80, "angular"): 25, (80, "cosine"): 5,
         (128, "angular"): 8, (128, "cosine"): 0}
MIN_GAP = 1e-5
REL = 2.0 ** -20


@pytest.fixture(scope="module")
def abx():
    import build_ext

    build_ext.build(verbose=False)
    import abx

    assert torch.cuda.is_available()
    abx.load_library()
    return abx


def distance_case(D, seed):
    """feats, start, len, grp_ptr: a group of 12 tokens, two of every length of LENGTHS in two rounds, so that the pairs (i, j),
    i < j, hold every ordered combination of lengths; a group of one token; a group of two; a group of 37 short tokens that
    overlap each other and the long ones."""
    rng = np.random.default_rng(1000 * D + seed)
    lens = list(LENGTHS) * 2
    start = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
    n_frames = int(np.sum(lens))
    lens += [5, 9, 4]
    start += [3, 40, 200]
    short = rng.integers(1, 13, 37)
    lens += short.tolist()
    start += [int(rng.integers(0, n_frames - n + 1)) for n in short]
    feats = rng.standard_normal((n_frames, D)).astype(np.float32)
    return feats, np.asarray(start, dtype=np.int64), np.asarray(lens, dtype=np.int32), np.array([0, 12, 13, 15, 52], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def oracle_case(D, metric, seed):
    feats, start, lens, grp = distance_case(D, seed)
    blocks, gaps = [], []
    for g in range(len(grp) - 1):
        b, gp = R.group_matrix(feats, start[grp[g]:grp[g + 1]], lens[grp[g]:grp[g + 1]], metric)
        blocks.append(b)
        gaps.append(gp)
    return blocks, min(float(g.min()) for g in gaps)


def run(abx, feats, start, lens, grp, metric, **kw):
    """-> (the groups' blocks as numpy, the status word)"""
    dev = torch.device("cuda:0")
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = abx.dtw(torch.from_numpy(feats).to(dev), torch.from_numpy(start).to(dev), torch.from_numpy(lens).to(dev), grp,
                  abx.METRICS[metric], status, **kw)
    host, n = out.cpu().numpy(), np.diff(grp)
    op = np.concatenate([[0], np.cumsum(n * n)])
    return [host[op[g]:op[g + 1]].reshape(n[g], n[g]) for g in range(len(n))], int(status.item())


def compare(got, want, exact_share):
    """|got - want| <= 2^-20 want everywhere, and at least exact_share of the pairs bitwise equal."""
    equal = total = 0
    for g, w in zip(got, want):
        assert g.shape == w.shape
        assert np.all(np.abs(g.astype(np.float64) - w.astype(np.float64)) <= REL * w.astype(np.float64))
        iu = np.triu_indices(w.shape[0], 1)
        equal += int((g.view(np.int32)[iu] == w.view(np.int32)[iu]).sum())
        total += len(iu[0])
    print("bitwise equal: %d of %d pairs" % (equal, total))
    assert equal >= exact_share * total


# --------------------------------------------------------------------------------------------------------------- distances
@pytest.mark.parametrize("D,metric", sorted(SEEDS))
def test_distances_against_oracle(abx, D, metric):
    """The arithmetic is mirrored, so only a cost on a float64 rounding boundary may differ (by one f32 ulp); such a cost must
    not redirect the path, which the oracle's gaps exclude first."""
    seed = SEEDS[(D, metric)]
    want, gap = oracle_case(D, metric, seed)
    assert gap >= MIN_GAP, gap
    feats, start, lens, grp = distance_case(D, seed)
    got, st = run(abx, feats, start, lens, grp, metric)
    assert st == 0
    compare(got, want, 0.99)


@pytest.mark.parametrize("metric", ["angular", "cosine"])
def test_distances_one_feature(abx, metric):
    """D = 1: every cosine is exactly +1 or -1 and every cost exactly 0 or 1 (0 or 2), so equal predecessors are the rule and
    no seed leaves a gap between them: the gap assertion cannot be made here.  It is not needed either: exact costs leave no
    rounding to differ in, the stated tie order decides alike on both sides, and every pair must be bitwise equal."""
    want, gap = oracle_case(1, metric, 0)
    assert gap == 0.0
    feats, start, lens, grp = distance_case(1, 0)
    got, st = run(abx, feats, start, lens, grp, metric)
    assert st == 0
    compare(got, want, 1.0)


def test_zero_row_and_identical_tokens(abx):
    rng = np.random.default_rng(7)
    feats = rng.standard_normal((30, 5)).astype(np.float32)
    feats[4] = 0.0
    feats[20] = 0.0
    #        a zero row alone, a row, a token around the zero row, the same again, a zero row alone again, a token twice
    start = np.array([4, 9, 2, 2, 20, 10, 10], dtype=np.int64)
    lens = np.array([1, 1, 6, 6, 1, 5, 5], dtype=np.int32)
    grp = np.array([0, 7], dtype=np.int64)
    for metric, zero_cost in (("angular", 0.5), ("cosine", 1.0)):
        got, st = run(abx, feats, start, lens, grp, metric)
        want, _ = R.group_matrix(feats, start, lens, metric)
        assert st == 0
        compare(got, [want], 0.99)
        # cos := 0 against a zero row, and between two zero rows
        assert got[0][0, 1] == np.float32(zero_cost) and got[0][0, 4] == np.float32(zero_cost)
        # identical tokens: the diagonal path; its costs are acos of a cosine within a rounding of 1, not exactly 0
        assert 0.0 <= got[0][5, 6] <= 1e-6 and got[0][5, 6] == want[5, 6]
        # ... and through a zero row, where cos := 0 holds against itself too: one cell of the six costs zero_cost
        assert got[0][2, 3] == want[2, 3] and abs(got[0][2, 3] - zero_cost / 6) <= 1e-6


# --------------------------------------------------------------------------------------------------------------- structure
def test_symmetry_diagonal_and_invariance(abx):
    feats, start, lens, grp = distance_case(32, 0)
    got, st = run(abx, feats, start, lens, grp, "angular")
    assert st == 0
    for b in got:
        assert np.array_equal(b.view(np.int32), b.T.view(np.int32))
        assert np.all(np.diag(b).view(np.int32) == 0)  # +0.0, written and not computed
        off = b[~np.eye(len(b), dtype=bool)]
        assert np.all(off > 0) and np.all(np.isfinite(off))
    # the last group (overlapping tokens) alone, and with the groups in another order
    a, b_ = int(grp[3]), int(grp[4])
    alone, st = run(abx, feats, start[a:b_], lens[a:b_], np.array([0, b_ - a]), "angular")
    assert st == 0 and np.array_equal(alone[0].view(np.int32), got[3].view(np.int32))
    order = np.concatenate([np.arange(a, b_), np.arange(0, 12), np.arange(13, 15), np.arange(12, 13)])
    moved, st = run(abx, feats, start[order], lens[order], np.array([0, 37, 49, 51, 52]), "angular")
    assert st == 0
    for m, g in zip(moved, (got[3], got[0], got[2], got[1])):
        assert np.array_equal(m.view(np.int32), g.view(np.int32))
    # its tokens permuted: the same distances at the permuted places, d(i, j) = d(j, i) included
    perm = np.random.default_rng(3).permutation(b_ - a)
    mixed, st = run(abx, feats, start[a:b_][perm], lens[a:b_][perm], np.array([0, b_ - a]), "angular")
    assert st == 0 and np.array_equal(mixed[0].view(np.int32), got[3][np.ix_(perm, perm)].view(np.int32))


def test_length_bound_changes_no_bit(abx):
    """max_len chooses the kernel instance (16, 32 or 64 rows of on-chip memory per token), not the values."""
    feats, start, lens, grp = distance_case(80, 0)
    a, b = int(grp[3]), int(grp[4])  # the 37 tokens of 1 .. 12 frames
    assert lens[a:b].max() <= 12
    one = np.array([0, b - a])
    ref, st = run(abx, feats, start[a:b], lens[a:b], one, "cosine")
    assert st == 0
    for bound in (12, 16, 17, 32, 33):
        got, st = run(abx, feats, start[a:b], lens[a:b], one, "cosine", max_len=bound)
        assert st == 0 and np.array_equal(got[0].view(np.int32), ref[0].view(np.int32)), bound
    # 17 and 63 frames under the middle and the full instance
    idx = np.array([3, 9, 0, 1, 2])
    ref, st = run(abx, feats, start[idx], lens[idx], np.array([0, 5]), "angular")
    got, st2 = run(abx, feats, start[idx], lens[idx], np.array([0, 5]), "angular", max_len=17)
    assert st == 0 and st2 == 0 and np.array_equal(got[0].view(np.int32), ref[0].view(np.int32))
    # a token above the bound is refused
    dev = torch.device("cuda:0")
    out = torch.full((25,), float("nan"), device=dev)
    _, st = run(abx, feats, start[idx], lens[idx], np.array([0, 5]), "angular", max_len=16, out=out)
    assert st == abx.ABX_BAD_TOKEN and bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------------------------ status
def test_status_bits_leave_out_untouched(abx):
    feats, start, lens, grp = distance_case(3, 0)
    dev = torch.device("cuda:0")

    good_out, good_pair = abx.group_ptrs(grp)

    def attempt(start, lens, grp, **kw):
        out = torch.full((int(good_out[-1]),), float("nan"), device=dev)  # NaN-prefilled: whatever is written shows
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        abx.dtw(torch.from_numpy(feats).to(dev), torch.from_numpy(start).to(dev), torch.from_numpy(lens).to(dev), grp, abx.ABX_ANGULAR,
                status, out=out, **kw)
        assert bool(torch.isnan(out).all())
        return int(status.item())

    for bad_len in (0, 65, -1):
        lens2 = lens.copy()
        lens2[20] = bad_len
        assert attempt(start, lens2, grp) == abx.ABX_BAD_TOKEN
    for bad_start in (feats.shape[0], feats.shape[0] - int(lens[14]) + 1, -1):
        start2 = start.copy()
        start2[14] = bad_start
        assert attempt(start2, lens, grp) == abx.ABX_BAD_TOKEN
    out_ptr = good_out.copy()
    out_ptr[2] += 1
    assert attempt(start, lens, grp, out_ptr=out_ptr) == abx.ABX_BAD_PTR
    pair_ptr = good_pair.copy()
    pair_ptr[-1] -= 1
    assert attempt(start, lens, grp, pair_ptr=pair_ptr) == abx.ABX_BAD_PTR
    # grp_ptr not monotone, not ending at N, not starting at 0 (against the pointers of the right one)
    for bad_grp in (np.array([0, 12, 11, 15, 52]), np.array([0, 12, 13, 15, 51]), np.array([1, 12, 13, 15, 52])):
        assert attempt(start, lens, bad_grp, out_ptr=good_out, pair_ptr=good_pair) == abx.ABX_BAD_PTR
    lens2, start2 = lens.copy(), start.copy()
    lens2[0], start2[51] = 0, -7
    assert attempt(start2, lens2, grp, out_ptr=out_ptr) == abx.ABX_BAD_TOKEN | abx.ABX_BAD_PTR
    # the status word is only ORed into
    status = torch.full((1,), 8, dtype=torch.int32, device=dev)
    abx.dtw(torch.from_numpy(feats).to(dev), torch.from_numpy(start).to(dev), torch.from_numpy(lens).to(dev), grp, 0, status)
    assert int(status.item()) == 8


def test_no_token_launches_nothing(abx):
    dev = torch.device("cuda:0")
    feats = torch.zeros(4, 3, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = abx.dtw(feats, torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), np.array([0]), 0,
                  status)
    assert out.shape == (0,) and int(status.item()) == 0
    out = abx.dtw(feats, torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), np.array([0, 0, 0]),
                  0, status)
    assert out.shape == (0,) and int(status.item()) == 0
    # an empty group among others is allowed
    got, st = run(abx, np.eye(4, 3, dtype=np.float32), np.array([0, 1], dtype=np.int64), np.array([2, 3], dtype=np.int32),
                  np.array([0, 0, 2, 2]), "cosine")
    assert st == 0 and got[0].shape == (0, 0) and got[1].shape == (2, 2) and got[1][0, 1] == got[1][1, 0] > 0


# ------------------------------------------------------------------------------------------------------------------ scores
PLANTED_SEED = 0
#: the oracle's scores on the planted data (checked below): within < across < 0.5
PLANTED_WITHIN, PLANTED_ACROSS = 0.0625, 0.185796


@functools.lru_cache(maxsize=None)
def planted(seed=PLANTED_SEED):
    """About 60 tokens of 3 phones in 2 contexts by 3 speakers: a per-phone template of 8 frames, time-warped to 5 .. 12 frames,
    plus a per-speaker offset and noise.  -> feats, tokens (abx.tokens_from_items' layout)."""
    rng = np.random.default_rng(seed)
    D, P, S, C = 8, 3, 3, 2
    templates = rng.standard_normal((P, 8, D))
    offsets = 0.9 * rng.standard_normal((S, D))
    rows, start, lens, phone, ctx, spk = [], [], [], [], [], []
    at = 0
    for k in range(60):
        p, c, s = k % P, (k // P) % C, (k // (P * C) + k) % S
        n = int(rng.integers(5, 13))
        warp = np.sort(rng.integers(0, 8, n))
        rows.append(templates[p][warp] + offsets[s] + 0.5 * rng.standard_normal((n, D)))
        start.append(at), lens.append(n), phone.append(p), ctx.append(c), spk.append(s)
        at += n
    tokens = {"start": np.asarray(start, dtype=np.int64), "len": np.asarray(lens, dtype=np.int32), "phone": np.asarray(phone),
              "ctx": np.asarray(ctx), "spk": np.asarray(spk), "phones": ["p0", "p1", "p2"], "contexts": [("a", "b"), ("c", "d")],
              "speakers": ["s0", "s1", "s2"], "dropped": {}}
    return np.concatenate(rows).astype(np.float32), tokens


@functools.lru_cache(maxsize=None)
def planted_oracle(seed=PLANTED_SEED):
    feats, t = planted(seed)
    N = len(t["start"])
    d = np.zeros((N, N), dtype=np.float32)
    for c in (0, 1):
        idx = np.nonzero(t["ctx"] == c)[0]
        d[np.ix_(idx, idx)] = R.group_matrix(feats, t["start"][idx], t["len"][idx], "angular")[0]
    return R.abx_triples(lambda a, b: d[a, b], t["phone"], t["ctx"], t["spk"])


def test_scores_on_planted_data(abx):
    feats, tokens = planted()
    want = planted_oracle()
    # no comparison the score rests on is close enough for an f32 ulp to turn it
    cmp = np.asarray(want["compared"], dtype=np.float64)
    assert np.all(np.abs(cmp[:, 0] - cmp[:, 1]) >= 1e-5 * np.maximum(cmp[:, 0], cmp[:, 1]))
    assert want["within"] == pytest.approx(PLANTED_WITHIN, abs=5e-7) and want["across"] == pytest.approx(PLANTED_ACROSS, abs=5e-7)
    assert want["within"] < want["across"] < 0.5
    dev_feats = torch.from_numpy(feats).cuda()
    got = abx.abx_scores(abx.pair_distances(dev_feats, tokens, "angular"), tokens)
    small = abx.abx_scores(abx.pair_distances(dev_feats, tokens, "angular", max_block_elems=900), tokens)  # one context per call
    for res in (got, small):
        for task in ("within", "across"):
            for key in ("cells_", "triples_", "gt_", "eq_"):
                assert res[key + task] == want[key + task], key + task
            assert abs(res[task] - want[task]) <= 1e-12
    assert got["tokens"] == 60
    with pytest.raises(ValueError, match=r"\('a', 'b'\)"):
        list(abx.pair_distances(dev_feats, tokens, "angular", max_block_elems=899))


# --------------------------------------------------------------------------------------------------------------------- CLI
def test_eval_model_cli(abx, tmp_path):
    import eval_model as EM
    import utils
    from fhvae import FHVAE

    T, F, H, D = 20, 16, 32, 16
    rs = np.random.RandomState(3)
    keys, items = [], []
    phones = ["aa", "iy", "s"]
    with open(tmp_path / "feats.scp", "w") as fs, open(tmp_path / "len.scp", "w") as ls:
        for s in range(2):
            for u in range(3):
                key, n = "s%02d-1-%04d" % (s + 1, u), 60 + 7 * u
                np.save(tmp_path / (key + ".npy"), (rs.randn(n, F) + s).astype(np.float32))
                fs.write("%s %s\n" % (key, tmp_path / (key + ".npy")))
                ls.write("%s %d\n" % (key, n))
                keys.append(key)
                for k in range(6):  # tokens of 6 frames, 3 phones, one context
                    items.append((key, 0.08 * k, 0.08 * k + 0.05, phones[(k + u) % 3], "b", "k", "s%02d" % (s + 1)))
    items.append(("nobody", 0.0, 0.1, "aa", "b", "k", "s01"))
    items.append((keys[0], 5.0, 5.1, "aa", "b", "k", "s01"))
    abx.write_items(str(tmp_path / "t.item"), items)
    torch.manual_seed(5)
    m = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, num_seqs=len(keys))
    utils.save_checkpoint(m, None, [], {}, "t", 1, 1, 0.0, 0.0, str(tmp_path))
    base = ["--checkpoint", str(tmp_path / "fhvae_t_e1.tar"), "--feat-scp", str(tmp_path / "feats.scp"), "--len-scp", str(tmp_path / "len.scp"),
            "--max-recon", "2"]
    plain, with_abx, only = tmp_path / "plain", tmp_path / "abx", tmp_path / "only"
    assert EM.main(base + ["--out", str(plain)]) == 0
    assert EM.main(base + ["--out", str(with_abx), "--abx-item", str(tmp_path / "t.item")]) == 0
    s_plain, s_abx = json.load(open(plain / "summary.json")), json.load(open(with_abx / "summary.json"))
    assert "abx" not in s_plain and sorted(p.name for p in plain.iterdir()) == sorted(
        p.name for p in with_abx.iterdir() if not p.name.startswith("abx_"))
    block = s_abx.pop("abx")
    assert set(s_abx) == set(s_plain) and s_abx["segments"] == s_plain["segments"] and s_abx["sequences"] == s_plain["sequences"]
    assert set(block) == {"z1", "feats", "tokens", "dropped", "distance", "frame_shift", "frame_offset"}
    assert block["tokens"] == 36 and block["distance"] == "angular" and block["frame_shift"] == 0.010 and block["frame_offset"] == 0.0
    assert block["dropped"] == {"unknown_utterance": 1, "no_frames": 1, "too_long": 0, "over_cell_cap": 0}
    for on in ("z1", "feats"):
        b = block[on]
        assert set(b) == {"within", "across", "cells_within", "cells_across", "triples_within", "triples_across"}
        assert 0.0 <= b["within"] <= 1.0 and 0.0 <= b["across"] <= 1.0
        # 2 speakers x 3 phones x 6 tokens: within, per speaker 6 ordered phone pairs of 6 * 5 * 6 triples; across, 6 * 6 * 6
        assert b["cells_within"] == 12 and b["triples_within"] == 12 * 180 and b["cells_across"] == 12 and b["triples_across"] == 12 * 216
        lines = open(with_abx / ("abx_by_pair_%s.tsv" % on)).read().splitlines()
        assert len(lines) == 1 + 6 and lines[0] == "phone\tother\twithin\tacross"
    assert EM.main(base + ["--out", str(only), "--abx-item", str(tmp_path / "t.item"), "--abx-on", "feats", "--abx-distance", "cosine",
                           "--abx-frame-offset", "0.0125", "--abx-max-per-cell", "2"]) == 0
    block = json.load(open(only / "summary.json"))["abx"]
    assert "z1" not in block and block["distance"] == "cosine" and block["tokens"] == 12 and block["dropped"]["over_cell_cap"] == 24
    assert not (only / "abx_by_pair_z1.tsv").exists() and (only / "abx_by_pair_feats.tsv").exists()
