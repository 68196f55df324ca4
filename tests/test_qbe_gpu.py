"""Query-by-example search on the GPU: fhvae_qbe_sdtw against the scalar oracle (tests/qbe_ref.py) over the shapes at which the
kernel takes another path, its invariance (batch, order, max_qlen, profile pointers, aliasing), its status word, qbe.search +
rank_metrics on planted terms, and the command lines search_terms.py and eval_model.py --qbe-queries."""
import functools
import json

import numpy as np
import pytest
import torch

import qbe_ref as R

pytestmark = pytest.mark.gpu

W = 64  # the kernel's column tile (csrc/qbe.hip, kQbeW)
Q_LENGTHS = (1, 2, 17, 63, 64)
U_LENGTHS = (1, 2, W - 1, 0, W, W + 1, 2 * W + 1, 300)  # an empty utterance in the middle
#: (D, metric) -> seed, chosen on the CPU so that the oracle alone leaves out at most MAX_LEFT_OUT of a case's columns and has
#: no near-tied best
SEEDS = {(3, "angular"): 0, (3, "cosine"): 0, (32, "angular"): 0, (32, "cosine"): 0, (80, "angular"): 0, (80, "cosine"): 0,
         (128, "angular"): 0, (128, "cosine"): 0}
MIN_GAP = 1e-5       # test_abx_gpu.py's
REL = 2.0 ** -20     # test_abx_gpu.py's
NEAR = 2.0 ** -19    # two end columns closer than this (relative) may swap as the best
MAX_LEFT_OUT = 0.10


@pytest.fixture(scope="module")
def qbe():
    import build_ext

    build_ext.build(verbose=False)
    import qbe

    assert torch.cuda.is_available()
    qbe.load_library()
    return qbe


def grid_case(D, seed):
    """qfeats, q_start, q_len, feats, utt_ptr: one query of every length of Q_LENGTHS, one utterance of every length of
    U_LENGTHS; contiguous rows."""
    rng = np.random.default_rng(1000 * D + seed)
    q_len = np.asarray(Q_LENGTHS, dtype=np.int32)
    q_start = np.concatenate([[0], np.cumsum(q_len)[:-1]]).astype(np.int64)
    utt_ptr = np.concatenate([[0], np.cumsum(U_LENGTHS)]).astype(np.int64)
    qfeats = rng.standard_normal((int(q_len.sum()), D)).astype(np.float32)
    feats = rng.standard_normal((int(utt_ptr[-1]), D)).astype(np.float32)
    return qfeats, q_start, q_len, feats, utt_ptr


@functools.lru_cache(maxsize=None)
def oracle_case(D, metric, seed):
    """-> e, s, gap (Q, n_frames) over the columns of every utterance"""
    qfeats, q_start, q_len, feats, utt_ptr = grid_case(D, seed)
    Q, n = len(q_len), len(feats)
    e, s, gap = np.zeros((Q, n), np.float32), np.zeros((Q, n), np.int64), np.zeros((Q, n))
    for q in range(Q):
        for u in range(len(utt_ptr) - 1):
            a, b = int(utt_ptr[u]), int(utt_ptr[u + 1])
            if b > a:
                e[q, a:b], s[q, a:b], gap[q, a:b] = R.sdtw(qfeats[q_start[q]:q_start[q] + q_len[q]], feats[a:b], metric)
    return e, s, gap


def run(qbe, qfeats, q_start, q_len, feats, utt_ptr, metric, alias=False, **kw):
    """-> (the five outputs as numpy, None where not asked for; the status word)"""
    dev = torch.device("cuda:0")
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    f = torch.from_numpy(feats).to(dev)
    out = qbe.sdtw(f if alias else torch.from_numpy(qfeats).to(dev), torch.from_numpy(q_start).to(dev), torch.from_numpy(q_len).to(dev), f,
                   torch.from_numpy(np.asarray(utt_ptr, dtype=np.int64)).to(dev), qbe.METRICS[metric], status, **kw)
    return [None if t is None else t.cpu().numpy() for t in out], int(status.item())


def bits(a):
    return a.view(np.int32)


def compare_grid(got, want, utt_ptr, compared_share, exact_share):
    """The rules of test_grid_against_oracle's docstring, and those of the best end: it is a column whose oracle e lies within
    NEAR of the smallest, the oracle's own wherever no second column does (near-tied cells: at most 1 %), and best_cost and
    best_start are the profile's values there."""
    best_cost, best_start, best_end, end_cost, end_start = got
    e, s, gap = want
    Q, n = e.shape
    cols = np.concatenate([np.arange(b - a) for a, b in zip(utt_ptr[:-1], utt_ptr[1:])])  # a column's frame in its utterance
    keep = gap >= MIN_GAP
    print("left out: %d of %d columns" % ((~keep).sum(), keep.size))
    assert (~keep).sum() <= (1.0 - compared_share) * keep.size
    assert np.all(np.isfinite(end_cost)) and np.all(end_start >= 0) and np.all(end_start <= cols[None, :])
    g64, w64 = end_cost.astype(np.float64), e.astype(np.float64)
    assert np.all(np.abs(g64 - w64)[keep] <= REL * w64[keep])
    equal = int((bits(end_cost) == bits(e))[keep].sum())
    print("bitwise equal: %d of %d compared columns" % (equal, keep.sum()))
    assert equal >= exact_share * keep.sum()
    assert np.array_equal(end_start[keep], s[keep])
    near_tied = cells = 0
    for q in range(Q):
        for u, (a, b) in enumerate(zip(utt_ptr[:-1], utt_ptr[1:])):
            if b == a:
                assert np.isposinf(best_cost[q, u]) and best_start[q, u] == -1 and best_end[q, u] == -1
                continue
            cells += 1
            j, ej = R.best(e[q, a:b])
            close = np.nonzero(w64[q, a:b] <= (1.0 + NEAR) * float(ej))[0]
            assert best_end[q, u] in close
            if len(close) > 1:
                near_tied += 1
            else:
                assert best_end[q, u] == j
            assert bits(best_cost)[q, u] == bits(end_cost)[q, a + best_end[q, u]] and best_start[q, u] == end_start[q, a + best_end[q, u]]
    print("near-tied best: %d of %d cells" % (near_tied, cells))
    assert near_tied <= 0.01 * cells


# ------------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("D,metric", sorted(SEEDS))
def test_grid_against_oracle(qbe, D, metric):
    """Every end column of 5 x 7 cells: query lengths 1 .. 64 against utterances of 1, 2, W - 1, W, W + 1, 2 W + 1 and 300 frames
    (shorter than the query, one tile, a tile boundary, several tiles) and an empty one.  The arithmetic is mirrored, so only
    a cost on a float64 rounding boundary may differ (by one f32 ulp); such a cost must not redirect a path, so the columns whose
    oracle path has a gap below MIN_GAP are left out (at most 10 % of them, asserted) and must only be finite with a start in
    [0, j]; on the others the cost is within 2^-20, bitwise equal in 99 % of them, and the start is equal."""
    seed = SEEDS[(D, metric)]
    qfeats, q_start, q_len, feats, utt_ptr = grid_case(D, seed)
    got, st = run(qbe, qfeats, q_start, q_len, feats, utt_ptr, metric, profile=True)
    assert st == 0
    compare_grid(got, oracle_case(D, metric, seed), utt_ptr, 1.0 - MAX_LEFT_OUT, 0.99)


@pytest.mark.parametrize("metric", ["angular", "cosine"])
def test_grid_one_feature(qbe, metric):
    """D = 1: every cosine is exactly +1 or -1 and every cost exactly 0 or 1 (0 or 2), so equal predecessors are the rule and no
    gap rule can apply.  None is needed: exact costs leave no rounding to differ in, the stated tie order decides alike on both
    sides, and every column, start and best must be bitwise equal."""
    qfeats, q_start, q_len, feats, utt_ptr = grid_case(1, 0)
    e, s, gap = oracle_case(1, metric, 0)
    assert gap.min() == 0.0
    (best_cost, best_start, best_end, end_cost, end_start), st = run(qbe, qfeats, q_start, q_len, feats, utt_ptr, metric, profile=True)
    assert st == 0
    assert np.array_equal(bits(end_cost), bits(e)) and np.array_equal(end_start, s)
    for q in range(len(q_len)):
        for u, (a, b) in enumerate(zip(utt_ptr[:-1], utt_ptr[1:])):
            if b > a:
                j, ej = R.best(e[q, a:b])
                assert best_end[q, u] == j and bits(best_cost)[q, u] == bits(e)[q, a + j] and best_start[q, u] == s[q, a + j]
            else:
                assert np.isposinf(best_cost[q, u]) and best_start[q, u] == -1 and best_end[q, u] == -1


def test_zero_rows(qbe):
    """cos := 0 against a zero row, in the query and in the utterance."""
    rng = np.random.default_rng(4)
    feats = rng.standard_normal((40, 5)).astype(np.float32)
    feats[7] = 0.0
    qfeats = rng.standard_normal((6, 5)).astype(np.float32)
    qfeats[0] = 0.0
    q_start, q_len, utt_ptr = np.array([0, 1], dtype=np.int64), np.array([1, 5], dtype=np.int32), np.array([0, 40])
    for metric, zero_cost in (("angular", 0.5), ("cosine", 1.0)):
        (_, _, _, end_cost, end_start), st = run(qbe, qfeats, q_start, q_len, feats, utt_ptr, metric, profile=True)
        assert st == 0 and np.all(end_cost[0] == np.float32(zero_cost)) and end_start[0].tolist() == list(range(40))
        e, s, _ = R.sdtw(qfeats[1:6], feats, metric)
        assert np.array_equal(end_start[1], s) and np.all(np.abs(end_cost[1].astype(np.float64) - e) <= REL * e)


# -------------------------------------------------------------------------------------------------------------- invariance
def test_batch_order_bound_profile_and_alias_change_no_bit(qbe):
    rng = np.random.default_rng(9)
    D = 32
    u_len = [70, 0, 3, 130, 64]
    utt_ptr = np.concatenate([[0], np.cumsum(u_len)]).astype(np.int64)
    feats = rng.standard_normal((int(utt_ptr[-1]), D)).astype(np.float32)
    q_start, q_len = np.array([10, 100, 5], dtype=np.int64), np.array([5, 16, 12], dtype=np.int32)  # rows of feats: aliased, overlapping
    ref, st = run(qbe, None, q_start, q_len, feats, utt_ptr, "angular", alias=True, profile=True)
    assert st == 0 and ref[0].shape == (3, 5) and ref[3].shape == (3, len(feats))
    # the same rows through a second tensor
    copy, st = run(qbe, feats.copy(), q_start, q_len, feats, utt_ptr, "angular", profile=True)
    assert st == 0 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(copy, ref))
    # without the profile pointers
    plain, st = run(qbe, None, q_start, q_len, feats, utt_ptr, "angular", alias=True)
    assert st == 0 and plain[3] is None and plain[4] is None
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(plain[:3], ref[:3]))
    # under every instance
    for bound in (16, 17, 32, 33, 64):
        got, st = run(qbe, None, q_start, q_len, feats, utt_ptr, "angular", alias=True, profile=True, max_qlen=bound)
        assert st == 0 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, ref)), bound
    # the queries permuted
    perm = np.array([2, 0, 1])
    got, st = run(qbe, None, q_start[perm], q_len[perm], feats, utt_ptr, "angular", alias=True, profile=True)
    assert st == 0 and all(np.array_equal(bits(a), bits(b[perm])) for a, b in zip(got, ref))
    # a cell alone: query 1 against utterance 3, cut out of the corpus
    a, b = int(utt_ptr[3]), int(utt_ptr[4])
    alone, st = run(qbe, feats[100:116].copy(), np.array([0], dtype=np.int64), np.array([16], dtype=np.int32), feats[a:b].copy(),
                    np.array([0, b - a]), "angular", profile=True, max_qlen=16)
    assert st == 0
    for k in range(3):
        assert bits(alone[k])[0, 0] == bits(ref[k])[1, 3]
    assert np.array_equal(bits(alone[3])[0], bits(ref[3])[1, a:b]) and np.array_equal(alone[4][0], ref[4][1, a:b])


# ------------------------------------------------------------------------------------------------------------------ status
def test_status_bits_leave_outputs_untouched(qbe):
    qfeats, q_start, q_len, feats, utt_ptr = grid_case(3, 0)
    dev = torch.device("cuda:0")
    Q, U, n = len(q_len), len(utt_ptr) - 1, len(feats)

    def attempt(q_start, q_len, utt_ptr, **kw):
        out = (torch.full((Q, U), float("nan"), device=dev), torch.full((Q, U), -7, dtype=torch.int32, device=dev),
               torch.full((Q, U), -7, dtype=torch.int32, device=dev), torch.full((Q, n), float("nan"), device=dev),
               torch.full((Q, n), -7, dtype=torch.int32, device=dev))  # prefilled: whatever is written shows
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        qbe.sdtw(torch.from_numpy(qfeats).to(dev), torch.from_numpy(q_start).to(dev), torch.from_numpy(q_len).to(dev),
                 torch.from_numpy(feats).to(dev), torch.from_numpy(utt_ptr).to(dev), qbe.QBE_ANGULAR, status, out=out, **kw)
        st = int(status.item())
        if st:
            assert bool(torch.isnan(out[0]).all()) and bool(torch.isnan(out[3]).all())
            assert all(bool((t == -7).all()) for t in (out[1], out[2], out[4]))
        return st

    assert attempt(q_start, q_len, utt_ptr) == 0
    for bad_len in (0, 65, -1):
        lens2 = q_len.copy()
        lens2[2] = bad_len
        assert attempt(q_start, lens2, utt_ptr) == qbe.QBE_BAD_QUERY
    for bad_start in (len(qfeats), len(qfeats) - int(q_len[3]) + 1, -1):
        start2 = q_start.copy()
        start2[3] = bad_start
        assert attempt(start2, q_len, utt_ptr) == qbe.QBE_BAD_QUERY
    assert attempt(q_start, q_len, utt_ptr, max_qlen=63) == qbe.QBE_BAD_QUERY  # a query above the caller's bound
    for k, v in ((2, int(utt_ptr[1]) - 1), (0, 1), (U, n - 1), (U, n + 1)):  # not monotone, not from 0, not to n_frames
        ptr2 = utt_ptr.copy()
        ptr2[k] = v
        assert attempt(q_start, q_len, ptr2) == qbe.QBE_BAD_PTR, (k, v)
    lens2, ptr2 = q_len.copy(), utt_ptr.copy()
    lens2[0], ptr2[3] = 0, -5
    assert attempt(q_start, lens2, ptr2) == qbe.QBE_BAD_QUERY | qbe.QBE_BAD_PTR
    # the status word is only ORed into
    status = torch.full((1,), 8, dtype=torch.int32, device=dev)
    qbe.sdtw(torch.from_numpy(qfeats).to(dev), torch.from_numpy(q_start).to(dev), torch.from_numpy(q_len).to(dev),
             torch.from_numpy(feats).to(dev), torch.from_numpy(utt_ptr).to(dev), 0, status)
    assert int(status.item()) == 8
    with pytest.raises(RuntimeError, match="utt_ptr"):
        qbe.check_status(torch.full((1,), qbe.QBE_BAD_PTR, dtype=torch.int32, device=dev))


def test_no_query_launches_nothing(qbe):
    dev = torch.device("cuda:0")
    feats = torch.zeros(4, 3, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    none64, none32 = torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    out = qbe.sdtw(feats, none64, none32, feats, torch.tensor([0, 4], device=dev), 0, status, profile=True)
    assert out[0].shape == (0, 1) and out[3].shape == (0, 4) and int(status.item()) == 0
    out = qbe.sdtw(feats, torch.tensor([0], device=dev), torch.tensor([2], dtype=torch.int32, device=dev), feats,
                   torch.tensor([0], device=dev), 0, status)
    assert out[0].shape == (1, 0) and int(status.item()) == 0
    res = qbe.search(feats, {"start": np.zeros(0, np.int64), "len": np.zeros(0, np.int32)}, feats, np.array([0, 4]))
    assert res["best_cost"].shape == (0, 1)


# ----------------------------------------------------------------------------------------------------------------- planted
PLANT_D, PLANT_U = 8, 10


@functools.lru_cache(maxsize=None)
def planted(seed=0):
    """A corpus of PLANT_U utterances of 120 .. 160 frames of N(0, 1) rows.  Two terms, a template of 10 .. 14 frames each, are
    planted into three utterances each as time-warped (every row once or twice), noised (0.05 sigma) copies; a third term is
    three unrelated random stretches of 12 frames.  -> feats, utt_ptr, items (abx.read_items' layout, 10 ms frames), keys"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(120, 161, PLANT_U)
    utt_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    feats = rng.standard_normal((int(utt_ptr[-1]), PLANT_D)).astype(np.float32)
    keys = ["utt%02d" % u for u in range(PLANT_U)]
    items = []
    utts = rng.permutation(PLANT_U)
    for t in range(2):
        template = rng.standard_normal((int(rng.integers(10, 15)), PLANT_D))
        for u in utts[3 * t:3 * t + 3]:
            warp = np.repeat(np.arange(len(template)), rng.integers(1, 3, len(template)))
            at = int(rng.integers(0, lens[u] - len(warp) + 1))
            feats[utt_ptr[u] + at:utt_ptr[u] + at + len(warp)] = template[warp] + 0.05 * rng.standard_normal((len(warp), PLANT_D))
            items.append((keys[u], 0.01 * at, 0.01 * (at + len(warp) - 1), "term%d" % t, "-", "-", "spk"))
    for u in utts[6:9]:
        at = int(rng.integers(0, lens[u] - 12))
        items.append((keys[u], 0.01 * at, 0.01 * (at + 11), "noise", "-", "-", "spk"))
    return feats, utt_ptr, items, keys


@functools.lru_cache(maxsize=None)
def planted_oracle(seed=0):
    """-> {(query, utterance): (j, e[j], s[j], the runner-up's e)} for every planted query against its relevant utterances and
    for every unplanted query against every other utterance"""
    import qbe

    feats, utt_ptr, items, keys = planted(seed)
    q = qbe.queries_from_items(items, keys, np.diff(utt_ptr))
    out = {}
    for k in range(len(q["start"])):
        term = q["terms"][q["term"][k]]
        for u in range(PLANT_U):
            mates = [it for it in items if it[3] == term and it[0] == keys[u]]
            if u == q["utt"][k] or (term != "noise" and not mates):
                continue
            e, s, _ = R.sdtw(feats[q["start"][k]:q["start"][k] + q["len"][k]], feats[utt_ptr[u]:utt_ptr[u + 1]], "angular")
            j, ej = R.best(e)
            out[(k, u)] = (j, float(ej), int(s[j]), float(np.partition(e, 1)[1]))
    return out


def test_search_on_planted_terms(qbe):
    feats, utt_ptr, items, keys = planted()
    lens = np.diff(utt_ptr)
    queries = qbe.queries_from_items(items, keys, lens)
    truth = qbe.truth_from_items(items, keys, lens)
    assert len(queries["start"]) == 9 and queries["terms"] == ["term0", "term1", "noise"] and sum(queries["dropped"].values()) == 0
    dev_feats = torch.from_numpy(feats).cuda()
    grid = qbe.search(dev_feats, queries, dev_feats, utt_ptr)
    small = qbe.search(dev_feats, queries, dev_feats, utt_ptr, max_cells=3 * PLANT_U * 2)  # two queries per call
    with_profile = qbe.search(dev_feats, queries, dev_feats, utt_ptr, profile=True, max_cells=1)  # one query per call
    for k in ("best_cost", "best_start", "best_end"):
        assert np.array_equal(bits(grid[k]), bits(small[k])) and np.array_equal(bits(grid[k]), bits(with_profile[k]))
    assert with_profile["end_cost"].shape == (9, len(feats))
    want = planted_oracle()
    is_planted = np.array([queries["terms"][t] != "noise" for t in queries["term"]])
    # every planted query ranks its two planted utterances first and finds the token there
    sub = {k: (v[is_planted] if isinstance(v, np.ndarray) else v) for k, v in queries.items() if k != "id"}
    res = qbe.rank_metrics(grid["best_cost"][is_planted], grid["best_start"][is_planted], grid["best_end"][is_planted], sub, truth)
    assert abs(res.pop("p_at_10") - 2 / 9) <= 1e-12  # (2 relevant among 9 candidates)
    assert res == {"map": 1.0, "p_at_n": 1.0, "located": 1.0, "queries": 6, "no_target": 0}
    exact = 0
    for (k, u), (j, ej, sj, second) in want.items():
        assert abs(float(grid["best_cost"][k, u]) - ej) <= 2 * REL * ej
        if second > (1.0 + NEAR) * ej:  # the oracle's best is not near-tied: the span is the oracle's
            assert (grid["best_start"][k, u], grid["best_end"][k, u]) == (sj, j)
            exact += 1
        if is_planted[k]:  # the detection is the planted token, give or take a frame at either end
            tok = [it for it in items if it[0] == keys[u] and it[3] == queries["terms"][queries["term"][k]]][0]
            f, l = int(round(tok[1] * 100)), int(round(tok[2] * 100))
            assert abs(sj - f) <= 1 and abs(j - l) <= 1
    assert exact >= 0.9 * len(want)
    # the unplanted term: chance level, and inside the range the oracle's costs give for it
    noise = ~is_planted
    sub = {k: (v[noise] if isinstance(v, np.ndarray) else v) for k, v in queries.items() if k != "id"}
    got = qbe.rank_metrics(grid["best_cost"][noise], grid["best_start"][noise], grid["best_end"][noise], sub, truth)
    bounds = []
    for sign in (+1.0, -1.0):  # every near-tie decided against, then for, the relevant utterances
        cost = np.full((9, PLANT_U), np.inf)
        for (k, u), (j, ej, sj, _) in want.items():
            rel = any(it[0] == keys[u] and it[3] == "noise" for it in items)
            cost[k, u] = ej * (1.0 + sign * NEAR) if rel else ej
        bounds.append(qbe.rank_metrics(cost[noise], grid["best_start"][noise], grid["best_end"][noise], sub, truth)["map"])
    print("unplanted MAP %.4f in [%.4f, %.4f]" % (got["map"], bounds[0], bounds[1]))
    assert got["queries"] == 3 and bounds[0] - 1e-12 <= got["map"] <= bounds[1] + 1e-12 and bounds[1] < 0.9


# --------------------------------------------------------------------------------------------------------------------- CLI
QBE_KEYS = {"on", "queries", "dropped", "distance", "utterances", "frames"}
SCORE_KEYS = {"map", "p_at_n", "p_at_10", "located", "no_target"}


def test_search_terms_cli(qbe, tmp_path):
    import search_terms as ST
    from test_units_gpu import tiny_corpus

    base, keys, lens = tiny_corpus(tmp_path)  # 36 tokens of 6 frames, 3 terms, and one of an unknown utterance
    item = str(tmp_path / "t.item")
    plain, scored, other = tmp_path / "plain", tmp_path / "scored", tmp_path / "other"
    assert ST.main(base + ["--queries", item, "--out", str(plain), "--top", "3"]) == 0
    info = json.load(open(plain / "qbe.json"))
    assert set(info) == QBE_KEYS and info["on"] == "z1" and info["queries"] == 15 and info["distance"] == "angular"
    assert info["dropped"] == {"unknown_utterance": 1, "no_frames": 0, "too_long": 0, "over_term_cap": 21}
    assert info["utterances"] == 6 and info["frames"] == sum(lens)
    lines = [ln.split("\t") for ln in open(plain / "hits.tsv").read().splitlines()]
    assert lines[0] == ["query", "term", "rank", "utterance", "start", "end", "cost"] and len(lines) == 1 + 15 * 3
    for k, row in enumerate(lines[1:]):
        assert len(row) == 7 and int(row[2]) == k % 3 + 1 and row[3] in keys and row[0].rsplit("_", 1)[0] == row[1]
        assert 0.0 <= float(row[4]) <= float(row[5]) and float(row[6]) >= 0.0
    assert all(row[3] != keys[0] for row in lines[1:4])  # the first query was cut from the first utterance: no candidate
    assert [float(r[6]) for r in lines[1:4]] == sorted(float(r[6]) for r in lines[1:4])
    # scored against the same tokens, on the input features, every token a query
    assert ST.main(base + ["--queries", item, "--item", item, "--out", str(scored), "--on", "feats", "--distance", "cosine",
                           "--max-per-term", "0"]) == 0
    info = json.load(open(scored / "qbe.json"))
    assert set(info) == QBE_KEYS | SCORE_KEYS and info["on"] == "feats" and info["queries"] == 36 and info["distance"] == "cosine"
    assert info["no_target"] == 0 and info["map"] == 1.0 and info["p_at_n"] == 1.0 and 0.0 <= info["located"] <= 1.0  # (every utterance holds every term)
    # the queries cut from a second corpus (the same files): a query's own utterance is a candidate now, and the best one
    assert ST.main(base + ["--queries", item, "--query-feat-scp", str(tmp_path / "feats.scp"), "--query-len-scp", str(tmp_path / "len.scp"),
                           "--out", str(other), "--on", "feats", "--top", "1", "--max-per-term", "1"]) == 0
    lines = [ln.split("\t") for ln in open(other / "hits.tsv").read().splitlines()][1:]
    assert [r[1] for r in lines] == ["aa", "iy", "s"] and all(r[3] == keys[0] for r in lines)
    assert [(r[4], r[5]) for r in lines] == [("0.000", "0.050"), ("0.080", "0.130"), ("0.160", "0.210")] and all(float(r[6]) < 1e-3 for r in lines)
    assert ST.main(base + ["--queries", str(tmp_path / "none.item"), "--out", str(tmp_path / "bad")]) == 1


def test_eval_model_cli(qbe, tmp_path):
    import eval_model as EM
    from test_units_gpu import tiny_corpus

    base, keys, lens = tiny_corpus(tmp_path)
    base = base + ["--max-recon", "2"]
    item = str(tmp_path / "t.item")
    plain, with_qbe, only = tmp_path / "plain", tmp_path / "qbe", tmp_path / "only"
    assert EM.main(base + ["--out", str(plain)]) == 0
    assert EM.main(base + ["--out", str(with_qbe), "--qbe-queries", item, "--qbe-item", item]) == 0
    s_plain, s_qbe = json.load(open(plain / "summary.json")), json.load(open(with_qbe / "summary.json"))
    assert "qbe" not in s_plain and sorted(p.name for p in plain.iterdir()) == sorted(p.name for p in with_qbe.iterdir())
    block = s_qbe.pop("qbe")
    assert set(s_qbe) == set(s_plain) and s_qbe["segments"] == s_plain["segments"] and s_qbe["sequences"] == s_plain["sequences"]
    assert set(block) == {"z1", "feats", "queries", "dropped", "distance", "frame_shift", "frame_offset"}
    assert block["queries"] == 15 and block["distance"] == "angular" and block["frame_shift"] == 0.010 and block["frame_offset"] == 0.0
    assert block["dropped"] == {"unknown_utterance": 1, "no_frames": 0, "too_long": 0, "over_term_cap": 21}
    for on in ("z1", "feats"):
        assert set(block[on]) == SCORE_KEYS and block[on]["no_target"] == 0
        assert block[on]["map"] == 1.0 and 0.0 <= block[on]["located"] <= 1.0  # (every utterance holds every term)
    assert EM.main(base + ["--out", str(only), "--qbe-queries", item, "--qbe-item", item, "--qbe-on", "feats", "--qbe-distance", "cosine",
                           "--qbe-max-per-term", "2"]) == 0
    block = json.load(open(only / "summary.json"))["qbe"]
    assert "z1" not in block and block["distance"] == "cosine" and block["queries"] == 6 and block["dropped"]["over_term_cap"] == 30
    with pytest.raises(SystemExit):
        EM.main(base + ["--out", str(only), "--qbe-queries", item])  # the two flags come together


def test_eval_model_cli_with_a_baseline_archive(qbe, tmp_path):
    """--baseline-feat-scp is one more entry of the "qbe" block, as of the "abx" and "units" blocks: the scores of qbe.evaluate on
    the archive's rows."""
    import abx
    import eval_model as EM
    import kaldi_io_lite as K
    from test_units_gpu import tiny_corpus

    base, keys, lens = tiny_corpus(tmp_path)
    item = str(tmp_path / "t.item")
    rng = np.random.default_rng(2)
    mats = [(rng.standard_normal((n, 39)) + (k[1:3] == "02")).astype(np.float32) for k, n in zip(keys, lens)]
    K.write_ark_scp(str(tmp_path / "mfcc.ark"), str(tmp_path / "mfcc.scp"), zip(keys, mats))
    out = tmp_path / "with"
    assert EM.main(base + ["--max-recon", "2", "--out", str(out), "--qbe-queries", item, "--qbe-item", item, "--qbe-on", "feats",
                           "--baseline-feat-scp", str(tmp_path / "mfcc.scp")]) == 0
    block = json.load(open(out / "summary.json"))["qbe"]
    assert set(block) == {"feats", "mfcc", "queries", "dropped", "distance", "frame_shift", "frame_offset"}
    items = abx.read_items(item)
    queries, truth = qbe.queries_from_items(items, keys, lens), qbe.truth_from_items(items, keys, lens)
    rows = torch.from_numpy(np.concatenate(mats)).cuda()
    want, _ = qbe.evaluate(rows, queries, rows, qbe.utt_ptr_of(lens), truth, "angular")
    assert block["mfcc"] == {k: want[k] for k in SCORE_KEYS} and block["mfcc"] != block["feats"]
