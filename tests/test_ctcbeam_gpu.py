"""CTC prefix beam search on the device (csrc/ctcbeam.hip) against the float64 oracle of tests/ctcbeam_ref.py on the cases of
tests/ctcbeam_cases.py, whose margins tests/test_ctcbeam_cpu.py has vetted: every utterance's hypothesis exactly, its score within
5 T 2^-53 max(1, |oracle|); -inf inputs and the emptied beam; the status bits; bitwise repeatability; search, tune and recognise
on the generator's corpus; both command lines."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import ctcbeam_cases as K
import ctcbeam_ref as R
import viterbi_ref as VR
from trellis_cases import bits64, dev, ptr_of

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def cb():
    import build_ext

    build_ext.build(verbose=False)
    import ctcbeam

    assert torch.cuda.is_available()
    ctcbeam.load_library()
    return ctcbeam


def hyps_of(tokens, ptr):
    t, p = tokens.cpu().numpy(), ptr.cpu().numpy()
    return [t[a:b].tolist() for a, b in zip(p[:-1], p[1:])]


def run(cb, c, **kw):
    tokens, ptr, score, bits = cb.decode(dev(c["z"]), dev(K.ptr_of(c)), c["blank"], c["W"], c["table"], c["class_beam"], with_status=True, **kw)
    assert tokens.dtype == torch.int32 and ptr.dtype == torch.int64 and score.dtype == torch.float64
    return hyps_of(tokens, ptr), score.cpu().numpy(), bits


WORST = {"share": 0.0}


def compare(c, hyps, score, want_hyps, want_score):
    for u, T in enumerate(c["lengths"]):
        assert hyps[u] == want_hyps[u], (c["name"], u, T)
        if T == 0:
            assert score[u] == want_score[u]
            continue
        b = K.bound(T, want_score[u])
        share = abs(score[u] - want_score[u]) / b
        WORST["share"] = max(WORST["share"], share)
        assert share <= 1.0, (c["name"], u, T, score[u], want_score[u], share)


# --------------------------------------------------------------------------------------------------------------------- grid
@pytest.mark.parametrize("name", K.ALL)
def test_decode_against_the_oracle(cb, name):
    """No utterance is left out: the CPU test holds every case's decision margin at 100 bounds or more.  The recreate-* cases are
    the regime in which prefixes fall out and come back (identity by creation node fails them), never-fills the beams that
    never fill."""
    c = K.case(name)
    want_hyps, want_score, _, want_status, _ = K.oracle(name)
    hyps, score, bits = run(cb, c)
    assert bits == want_status == 0
    compare(c, hyps, score, want_hyps, want_score)
    print("%s: worst share of the score bound so far %.3f" % (name, WORST["share"]))


@pytest.mark.parametrize("with_table", [False, True])
def test_brute_force_on_the_device(cb, with_table):
    """T <= 5, C <= 3, W = 64: the search is exact, so the device's hypothesis is the best labelling of all C^T paths."""
    n = 0
    for z, blank, table in K.small(with_table):
        ranked = sorted(R.brute_force(z, blank, table).items(), key=lambda kv: -kv[1])
        T, C = z.shape
        tokens, ptr, score = cb.decode(dev(z.reshape(T, C)), dev(np.array([0, T])), blank, 64, table)
        got = float(score[0])
        assert abs(got - ranked[0][1]) <= 1e-12 * max(1.0, abs(got)), (z, blank, got, ranked[:2])
        if len(ranked) == 1 or ranked[0][1] - ranked[1][1] > 1e-9:
            assert tuple(hyps_of(tokens, ptr)[0]) == ranked[0][0]
            n += 1
    assert n >= 60


def test_tie_order_on_the_device(cb):
    z = np.array([[0.0, 1.0, 1.0, 1.0, 1.0]], np.float32)
    end = np.zeros((6, 6))
    end[2, 5], end[4, 5] = 1.0, 5.0
    for W, want in ((1, [1]), (2, [2]), (3, [2]), (4, [4]), (64, [4])):
        tokens, ptr, score = cb.decode(dev(z), dev(np.array([0, 1])), 0, W, end)
        assert hyps_of(tokens, ptr) == [want] and float(score[0]) == R.decode(z, 0, W, end)[1], W
    tokens, ptr, _ = cb.decode(dev(z), dev(np.array([0, 1])), 0, 2)
    assert hyps_of(tokens, ptr) == [[1]]


# ------------------------------------------------------------------------------------------------- -inf and the empty beam
def test_minus_infinity_inputs_and_the_empty_beam(cb):
    rng = np.random.default_rng(4)
    C, blank, W = 4, 1, 8
    z = rng.standard_normal((40, C)).astype(np.float32)
    lengths = [12, 9, 0, 19]
    ptr = ptr_of(lengths)
    # a class at probability 0 that the best labelling does not need, and one it would have needed
    want_plain = R.batch(z, ptr, blank, W)[0]
    for dead in range(C):
        if dead == blank:
            continue
        zd = z.copy()
        zd[:, dead] = -INF
        want = R.batch(zd, ptr, blank, W)
        tokens, hp, score, bits = cb.decode(dev(zd), dev(ptr), blank, W, with_status=True)
        assert bits == 0 and hyps_of(tokens, hp) == want[0] and all(dead not in h for h in want[0])
        assert np.allclose(score.cpu().numpy(), want[1], rtol=1e-13, atol=0)
    assert any(any(v in h for h in want_plain) for v in range(C) if v != blank)
    # a forbidden repeat and a forbidden start
    for forbid in ("repeat", "start"):
        tab = rng.standard_normal((C + 1, C + 1))
        if forbid == "repeat":
            tab[np.arange(C), np.arange(C)] = -INF
        else:
            tab[C, 0] = tab[C, 2] = -INF
        want = R.batch(z, ptr, blank, W, tab)
        tokens, hp, score, bits = cb.decode(dev(z), dev(ptr), blank, W, tab, with_status=True)
        got = hyps_of(tokens, hp)
        assert bits == 0 and got == want[0] and np.allclose(score.cpu().numpy(), want[1], rtol=1e-13, atol=0)
        if forbid == "repeat":
            assert all(a != b for h in got for a, b in zip(h[:-1], h[1:]))
        else:
            assert all(not h or h[0] == 3 for h in got)
    # the blank at probability 0 in utterance 1 and every start forbidden: its beam empties out at its first frame.  That
    # concerns utterance 1 only
    tab = np.zeros((C + 1, C + 1))
    tab[C, :C] = -INF
    ze = z.copy()
    ze[ptr[1]:ptr[2], blank] = -INF
    want = R.batch(ze, ptr, blank, W, tab)
    assert want[3] == R.EMPTY and want[0][1] == [] and want[1][1] == -INF
    tokens, hp, score, bits = cb.decode(dev(ze), dev(ptr), blank, W, tab, with_status=True)
    s = score.cpu().numpy()
    assert bits == cb.CB_EMPTY and hyps_of(tokens, hp) == want[0] == [[], [], [], []] and s[1] == -INF
    assert np.isfinite(s[[0, 3]]).all() and np.allclose(s[[0, 2, 3]], want[1][[0, 2, 3]], rtol=1e-13, atol=0) and s[2] == 0.0


# --------------------------------------------------------------------------------------------------- status and robustness
def raw(cb, z, ptr, C, blank, W, class_beam, lm, hyp, hyp_len, score, status, ws, n_frames=None, ws_bytes=None):
    import hip_binding as hb

    n_frames = int(z.shape[0]) if n_frames is None else n_frames
    hb._call("fhvae_cb_decode", hb._p(z), z.stride(0), n_frames, C, blank, hb._p(ptr), int(ptr.shape[0]) - 1, W, class_beam,
             hb._p(lm) if lm is not None else None, hb._p(hyp), hb._p(hyp_len), hb._p(score), hb._p(status), hb._p(ws),
             ws.numel() if ws_bytes is None else ws_bytes)
    torch.cuda.synchronize()


def test_padded_rows_sentinels_and_status_bits(cb):
    lib = cb.load_library()
    rng = np.random.default_rng(9)
    C, blank, W, lengths = 5, 2, 8, [7, 0, 11, 5]
    ptr, N = ptr_of(lengths), 23
    z = rng.standard_normal((N, C)).astype(np.float32)
    want = R.batch(z, ptr, blank, W)
    # rows with a leading dimension of 12: NaN in the columns past C, which no kernel may read
    wide = torch.full((N, 12), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :C] = dev(z)
    tokens, hp, score = cb.decode(wide[:, :C], dev(ptr), blank, W)
    assert hyps_of(tokens, hp) == want[0]
    base = bits64(score)
    # the raw call: outputs beyond what it may write keep their sentinel
    need = int(lib.fhvae_cb_ws_bytes(N, W))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def outputs():
        return (torch.full((N + 4,), -7, dtype=torch.int32, device="cuda"), torch.full((len(lengths) + 2,), -7, dtype=torch.int32, device="cuda"),
                torch.full((len(lengths) + 2,), -7.0, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))

    hyp, hyp_len, sc, status = outputs()
    raw(cb, wide, dev(ptr), C, blank, W, INF, None, hyp, hyp_len, sc, status, ws)
    assert int(status[0]) == 0 and hyp_len.cpu().tolist() == [len(h) for h in want[0]] + [-7, -7]
    assert np.array_equal(bits64(sc[:4]), base) and sc[4:].cpu().tolist() == [-7.0, -7.0]
    h = hyp.cpu().numpy()
    for u in range(4):
        a, L = int(ptr[u]), len(want[0][u])
        assert h[a:a + L].tolist() == want[0][u] and (h[a + L:int(ptr[u + 1])] == -7).all()
    assert (h[N:] == -7).all()
    # FHVAE_CB_BAD_PTR: nothing is written
    for bad in ([1, 7, 7, 18, 23], [0, 7, 6, 18, 23], [0, 7, 7, 18, 22], [0, 7, 7, 18, 24], [0, -1, 7, 18, 23]):
        hyp, hyp_len, sc, status = outputs()
        raw(cb, wide, dev(np.array(bad, dtype=np.int64)), C, blank, W, INF, None, hyp, hyp_len, sc, status, ws)
        assert int(status[0]) == cb.CB_BAD_PTR, bad
        assert (hyp == -7).all() and (hyp_len == -7).all() and (sc == -7.0).all(), bad
    with pytest.raises(RuntimeError, match="monotone"):
        cb.decode(dev(z), dev(np.array([0, 7, 6, 18, 23])), blank, W)
    # a status word that is not clear keeps its other bits
    hyp, hyp_len, sc, status = outputs()
    status.fill_(64)
    raw(cb, wide, dev(ptr), C, blank, W, INF, None, hyp, hyp_len, sc, status, ws)
    assert int(status[0]) == 64 and np.array_equal(bits64(sc[:4]), base)
    # the Python side refuses what it can before any C call
    for args in ((dev(z), dev(ptr), 5, W), (dev(z), dev(ptr), blank, 0), (dev(z), dev(ptr), blank, 65), (dev(z), dev(ptr[:-1]), blank, W)):
        with pytest.raises(RuntimeError):
            cb.decode(*args)
    with pytest.raises(RuntimeError, match="class_beam"):
        cb.decode(dev(z), dev(ptr), blank, W, None, -1.0)
    with pytest.raises(RuntimeError, match="lm"):
        cb.decode(dev(z), dev(ptr), blank, W, np.zeros((5, 5)))
    empty = cb.decode(dev(z[:0]), dev(np.array([0])), blank, W)
    assert empty[0].numel() == 0 and empty[1].cpu().tolist() == [0] and empty[2].numel() == 0


def test_a_nan_row_stays_in_its_utterance(cb):
    c = K.case("grid-C5-W16")
    base = cb.decode(dev(c["z"]), dev(K.ptr_of(c)), c["blank"], c["W"], c["table"], c["class_beam"])
    z = c["z"].copy()
    ptr = K.ptr_of(c)
    u = 5  # (64 frames)
    z[ptr[u] + 10, 1] = np.nan
    got = cb.decode(dev(z), dev(ptr), c["blank"], c["W"], c["table"], c["class_beam"])
    keep = np.array([v for v in range(len(c["lengths"])) if v != u])
    assert np.array_equal(bits64(got[2])[keep], bits64(base[2])[keep])
    a, b = hyps_of(got[0], got[1]), hyps_of(base[0], base[1])
    assert [a[v] for v in keep] == [b[v] for v in keep]


@pytest.mark.parametrize("name", ["grid-C3-W64", "grid-C61-W16", "grid-C128-W63", "recreate-lm"])
def test_an_utterance_does_not_depend_on_its_batch(cb, name):
    """Alone against in the batch, two leading dimensions, two workspace limits, run to run: the same bits."""
    c = K.case(name)
    ptr = K.ptr_of(c)
    z, table = dev(c["z"]), c["table"]
    tokens, hp, score = cb.decode(z, dev(ptr), c["blank"], c["W"], table, c["class_beam"])
    hyps, base = hyps_of(tokens, hp), bits64(score)
    again = cb.decode(z, dev(ptr), c["blank"], c["W"], table, c["class_beam"])
    assert hyps_of(again[0], again[1]) == hyps and np.array_equal(bits64(again[2]), base)
    wide = torch.full((z.shape[0], c["C"] + 11 - (c["C"] + 3) % 4), 3.0, dtype=torch.float32, device="cuda")
    assert wide.shape[1] % 4 == 0 and wide.shape[1] >= c["C"] + 4
    wide[:, :c["C"]] = z
    other = cb.decode(wide[:, :c["C"]], dev(ptr), c["blank"], c["W"], table, c["class_beam"])
    assert hyps_of(other[0], other[1]) == hyps and np.array_equal(bits64(other[2]), base)
    split = cb.decode(z, dev(ptr), c["blank"], c["W"], table, c["class_beam"], ws_limit=16 * c["W"] * 70)  # a few utterances a group
    assert hyps_of(split[0], split[1]) == hyps and np.array_equal(bits64(split[2]), base)
    for u, T in enumerate(c["lengths"]):
        alone = cb.decode(z[ptr[u]:ptr[u + 1]], dev(np.array([0, T])), c["blank"], c["W"], table, c["class_beam"])
        assert hyps_of(alone[0], alone[1]) == [hyps[u]] and bits64(alone[2])[0] == base[u], (name, u)


# --------------------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def corpus():
    c = VR.corpus(60, 5, 8, 1.3, 0)
    ptr = ptr_of(c["lengths"])
    return c, ptr, int(ptr[40])


def test_search_tune_and_recognise_on_the_generators_corpus(cb):
    """ctc.fit at context 2 on 40 utterances, 20 held out: beam 16 with the bigram tuned on the training utterances against
    ctc.greedy in the same test.  The CPU prototype of the issue had 0.089 against 0.210."""
    import ctc
    import phonerec

    c, ptr, cut = corpus()
    lens, names = c["lengths"], ["p%d" % i for i in range(5)]
    train_x, test_x, train_refs, test_refs = dev(c["x"][:cut]), dev(c["x"][cut:]), c["refs"][:40], c["refs"][40:]
    model, rep_greedy, hyp_greedy, ref = ctc.recognise(train_x, lens[:40], train_refs, test_x, lens[40:], test_refs, names, iters=60, context=2)
    same, rep, hyp, ref2, lm = cb.recognise(train_x, lens[:40], train_refs, test_x, lens[40:], test_refs, names, beam=16, model=model)
    assert same is model and ref2 == ref == test_refs and len(hyp) == 20
    assert np.array_equal(lm, cb.bigram(train_refs, 6, 5, 1.0)) and lm.shape == (7, 7)
    grid = rep["grid"]
    assert len(grid) == 16 and (rep["lm_scale"], rep["bonus"]) == cb.best_of(grid) and rep["beam"] == 16 and rep["class_beam"] is None
    assert rep["per"] == VR.per(ref, hyp)
    # search is what recognise decoded with; tune gives the grid again; without a table and at beam 1 nothing else changes
    test_ptr = dev(ptr_of(lens[40:]))
    tok, tp = cb.search(test_x, test_ptr, model, 16, lm, rep["lm_scale"], rep["bonus"])
    assert phonerec.uncsr(tok, tp) == hyp
    best, again = cb.tune(train_x, dev(ptr[:41]), train_refs, model, lm, 16)
    assert again == grid and best == (rep["lm_scale"], rep["bonus"])
    no_lm = VR.per(ref, phonerec.uncsr(*cb.search(test_x, test_ptr, model, 4)))
    fixed = cb.recognise(train_x, lens[:40], train_refs, test_x, lens[40:], test_refs, names, beam=4, scale=1.0, bonus=0.0, model=model)[1]
    assert fixed["grid"] is None and fixed["lm_scale"] == 1.0 and fixed["bonus"] == 0.0
    # the device's hypotheses on the model's logits are the oracle's
    z, _ = cb._logits("test", test_x, test_ptr, model)
    want = R.batch(z.cpu().numpy(), ptr_of(lens[40:]), 5, 16, cb.table(lm, rep["lm_scale"], rep["bonus"]))
    if want[2].min() > 1e-9:
        assert [h for h in want[0]] == hyp
    print("held-out PER at context 2: greedy %.4f, beam 4 no LM %.4f, beam 4 bigram x1 bonus 0 %.4f, beam 16 tuned (scale %g, bonus %g) %.4f; grid %s"
          % (rep_greedy["per"], no_lm, fixed["per"], rep["lm_scale"], rep["bonus"], rep["per"], grid))
    assert rep["per"] < rep_greedy["per"]


# --------------------------------------------------------------------------------------------------------------------- CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BEAM_KEYS = {"per", "sub", "del", "ins", "cor", "ref_tokens", "utterances", "beam", "lm_scale", "bonus", "class_beam", "smooth", "grid"}


def test_recognise_phones_cli_with_the_beam(cb, tmp_path, capsys):
    import recognise_phones as RP
    from test_ctc_gpu import same_content
    from test_gmm_gpu import feats_corpus

    base, keys, lens = feats_corpus(tmp_path)
    common = base + ["--item", str(tmp_path / "t.item"), "--on", "feats", "--iters", "30"]
    plain, with_c, with_b = tmp_path / "plain", tmp_path / "ctc", tmp_path / "beam"
    # without the new flags: what the command wrote before they existed
    assert RP.main(common + ["--out", str(plain)]) == 0
    info = json.load(open(plain / "phonerec.json"))
    same_content(info, json.load(open(GOLDEN + "/ctc_recognise_phones_plain.json")))
    assert (plain / "hyp.txt").read_text() == open(GOLDEN + "/ctc_recognise_phones_plain_hyp.txt").read()
    assert sorted(p.name for p in plain.iterdir()) == ["hyp.txt", "phonerec.json", "probe.npz", "ref.txt"]
    assert RP.main(common + ["--out", str(with_c), "--ctc"]) == 0
    assert RP.main(common + ["--out", str(with_b), "--ctc", "--ctc-beam", "8", "--ctc-lm-tune", "--ctc-class-beam", "20"]) == 0
    assert sorted(p.name for p in with_b.iterdir()) == ["ctc.npz", "ctc_lm.npy", "hyp.txt", "hyp_ctc.txt", "hyp_ctc_beam.txt", "phonerec.json",
                                                        "probe.npz", "ref.txt"]
    for name in ("hyp.txt", "ref.txt", "hyp_ctc.txt"):
        assert (with_b / name).read_bytes() == (with_c / name).read_bytes(), name
    for name in ("probe.npz", "ctc.npz"):
        with np.load(with_b / name) as a, np.load(with_c / name) as b:
            assert sorted(a.files) == sorted(b.files) and all(np.array_equal(a[k], b[k]) for k in a.files), name
    got = json.load(open(with_b / "phonerec.json"))
    block = got.pop("ctc_beam")
    assert got == json.load(open(with_c / "phonerec.json"))
    assert set(block) == BEAM_KEYS and block["beam"] == 8 and block["class_beam"] == 20.0 and len(block["grid"]) == 16
    assert block["sub"] + block["del"] + block["cor"] == block["ref_tokens"] == info["ref_tokens"]
    lm = np.load(with_b / "ctc_lm.npy")
    assert lm.shape == (6, 6) and np.isneginf(lm[4]).all()
    hyp = (with_b / "hyp_ctc_beam.txt").read_text().splitlines()
    assert [l.split()[0] for l in hyp] == [l.split()[0] for l in (plain / "ref.txt").read_text().splitlines()]
    assert set(t for l in hyp for t in l.split()[1:]) <= set(info["classes"])
    fixed = tmp_path / "fixed"
    assert RP.main(common + ["--out", str(fixed), "--ctc", "--ctc-beam", "4", "--ctc-lm-scale", "0.5", "--ctc-bonus", "1", "--ctc-lm-smooth", "0.5"]) == 0
    block = json.load(open(fixed / "phonerec.json"))["ctc_beam"]
    assert (block["beam"], block["lm_scale"], block["bonus"], block["smooth"], block["grid"]) == (4, 0.5, 1.0, 0.5, None)
    capsys.readouterr()
    for bad in (["--ctc-beam", "4"], ["--ctc", "--ctc-lm-scale", "1"], ["--ctc", "--ctc-beam", "65"], ["--ctc", "--ctc-beam", "4", "--ctc-lm-tune", "--ctc-bonus", "1"],
                ["--ctc", "--ctc-beam", "4", "--ctc-class-beam", "-1"]):
        with pytest.raises(SystemExit):
            RP.main(common + ["--out", str(tmp_path / "no")] + bad)


def test_per_ctc_beam_block_of_eval_model(cb, tmp_path):
    import eval_model as EM
    from test_ctc_gpu import same_content
    from test_units_gpu import tiny_corpus

    base, keys, lens = tiny_corpus(tmp_path)
    common = base + ["--max-recon", "2", "--per-item", str(tmp_path / "t.item"), "--probe-iters", "20"]
    plain, with_c, with_b = tmp_path / "plain", tmp_path / "with", tmp_path / "beam"
    assert EM.main(common + ["--out", str(plain)]) == 0
    per = json.load(open(plain / "summary.json"))["per"]
    want = json.load(open(GOLDEN + "/ctc_eval_model_per_plain.json"))
    same_content({k: v for k, v in per.items() if k != "z1"}, {k: v for k, v in want.items() if k != "z1"})
    assert set(per["z1"]) == set(want["z1"]) and per["z1"]["ref_tokens"] == want["z1"]["ref_tokens"]
    assert EM.main(common + ["--out", str(with_c), "--per-ctc"]) == 0
    assert EM.main(common + ["--out", str(with_b), "--per-ctc", "--per-ctc-beam", "8", "--per-ctc-lm-scale", "0.5"]) == 0
    got, ref = json.load(open(with_b / "summary.json"))["per"], json.load(open(with_c / "summary.json"))["per"]
    for on in ("z1", "feats"):
        block = got[on].pop("ctc_beam")
        assert set(block) == BEAM_KEYS and (block["beam"], block["lm_scale"], block["bonus"], block["grid"]) == (8, 0.5, 0.0, None)
        assert block["ref_tokens"] == got[on]["ref_tokens"] and block["per"] >= 0.0
    same_content(got["feats"], ref["feats"])
    assert set(got["z1"]) == set(ref["z1"])
    for bad in (["--per-ctc-beam", "4"], ["--per-ctc", "--per-ctc-bonus", "1"], ["--per-ctc", "--per-ctc-beam", "0"]):
        with pytest.raises(SystemExit):
            EM.main(common + ["--out", str(tmp_path / "no")] + bad)
