"""Forced alignment on the GPU: fhvae_fa_align against the float64 oracle of tests/falign_ref.py BIT FOR BIT -- state, seg and
score; there is no tolerance anywhere (the recursion holds float64 additions of f32 inputs, one rounding each, and exact maxima).
The grid covers the trace-back chunk edges (T), the states-per-lane edges (L) in both topologies, equal neighbours, the one-path
case and the infeasible one beside it, empty utterances between all of them; random scores at two scales, small integers and
all-zero rows (exact ties), a -inf class; padded rows with sentinel columns, sentinel-filled outputs under every status bit, a NaN
row, bitwise batch independence; falign.align on the generator's corpus, ctc.fit + alignment end to end, and align_phones.py."""
import functools
import json

import numpy as np
import pytest
import torch

import falign_ref as R
import viterbi_ref as VR
from trellis_cases import bits64, blank_of, dev, labels_for, ptr_of

pytestmark = pytest.mark.gpu

CLASSES = (2, 3, 64, 65, 128)
FRAMES = (1, 2, 63, 64, 65, 128, 129, 300)
LABELS = (0, 1, 2, 31, 32, 63, 64, 127, 128, 129, 256)
HMM_LABELS = (1, 2, 64, 65, 128, 129, 256)
KINDS = ("n1", "n50", "int", "zero", "ninf")
NEG = -np.inf


@pytest.fixture(scope="module")
def fa():
    import build_ext

    build_ext.build(verbose=False)
    import falign

    assert torch.cuda.is_available()
    falign.load_library()
    return falign


def fits(T, lab, blank):
    if blank < 0:
        return T >= len(lab) >= 1
    return T >= len(lab) + sum(1 for a, b in zip(lab[:-1], lab[1:]) if a == b)


def batch_of(shapes, C, blank, kind, rng):
    lens, labs = [0], [[]]
    for T, lab in shapes:  # an empty utterance before, between and after
        lens += [T, 0]
        labs += [lab, []]
    ptr, lab_ptr = ptr_of(lens), ptr_of([len(l) for l in labs])
    labels = np.concatenate([np.asarray(l, dtype=np.int32) for l in labs])
    N = int(ptr[-1])
    if kind == "int":
        z = rng.integers(-2, 3, size=(N, C)).astype(np.float32)
    elif kind == "zero":
        z = np.zeros((N, C), dtype=np.float32)
    else:
        z = ((50.0 if kind == "n50" else 1.0) * rng.standard_normal((N, C))).astype(np.float32)
    if kind == "ninf":  # a class no utterance can pass: some transcriptions need it, others do not
        z[:, [c for c in range(C) if c != blank][-1]] = NEG
    state, seg, score, status = R.batch(z, ptr, labels, lab_ptr, blank)
    return {"C": C, "blank": blank, "z": z, "ptr": ptr, "labels": labels, "lab_ptr": lab_ptr, "state": state, "seg": seg, "score": score,
            "status": status, "lens": np.asarray(lens), "labs": labs}


@functools.lru_cache(maxsize=None)
def case(C, where, kind):
    """One batch: every T of FRAMES with every L of the topology's list that fits, plain and with equal neighbours; an all-equal
    transcription at exactly T = 2 L - 1 (one path) and one frame short of it (CTC), T = L and T = L - 1 (HMM); no frame at all;
    the oracle's answers, once."""
    rng = np.random.default_rng(100 * C + 7 * len(where) + KINDS.index(kind))
    blank = blank_of(C, where)
    shapes = []
    for T in FRAMES:
        for L in (HMM_LABELS if blank < 0 else LABELS):
            for rep in (0, 2):
                lab = labels_for(rng, L, C, blank, rep)
                if (rep == 0 or L >= 3) and fits(T, lab, blank):
                    shapes.append((T, lab))
    same = [c for c in range(C) if c != blank][0]
    if blank < 0:
        shapes += [(64, labels_for(rng, 64, C, blank, 2)), (63, labels_for(rng, 64, C, blank, 2)), (129, [same] * 129), (128, [same] * 129),
                   (0, [same])]
    else:
        shapes += [(65, [same] * 33), (64, [same] * 33), (0, [same])]
    return batch_of(shapes, C, blank, kind, rng)


def run(fa, c, ws_limit=1 << 30, z=None):
    state, seg, score, bits = fa.align(dev(c["z"]) if z is None else z, dev(c["ptr"]), dev(c["labels"]), dev(c["lab_ptr"]), c["blank"],
                                       ws_limit=ws_limit)
    return state.cpu().numpy(), seg.cpu().numpy().reshape(-1), score.cpu().numpy(), bits


def same_bits(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(bits64(got[2]), bits64(want[2]))
            and got[3] == want[3])


def oracle(c):
    return c["state"], c["seg"], c["score"], c["status"]


# ------------------------------------------------------------------------------------------------------------------- kernel
GRID = ([(C, w, "n1") for C in CLASSES for w in ("first", "middle", "last", "hmm")]
        + [(C, w, k) for C, w in ((3, "first"), (65, "middle"), (128, "last"), (3, "hmm"), (65, "hmm")) for k in KINDS[1:]])


@pytest.mark.parametrize("C,where,kind", GRID)
def test_align_against_the_oracle(fa, C, where, kind):
    c = case(C, where, kind)
    state, seg, score, bits = run(fa, c)
    assert state.dtype == np.int32 and seg.dtype == np.int32 and score.dtype == np.float64
    feasible = np.isfinite(c["score"])
    print("C %d %s %s: %d utterances, %d with a path, %d frames" % (C, where, kind, len(c["score"]), int(feasible.sum()), len(c["state"])))
    assert feasible.sum() > 30 and (~feasible).sum() >= 2
    assert bits == c["status"] and bits & fa.FA_INFEASIBLE
    bad = np.nonzero(bits64(score) != bits64(c["score"]))[0]
    assert bad.size == 0, (bad[:5], score[bad[:5]], c["score"][bad[:5]])
    assert np.array_equal(state, c["state"]), np.nonzero(state != c["state"])[0][:10]
    assert np.array_equal(seg, c["seg"]), np.nonzero(seg != c["seg"])[0][:10]
    empty = (c["lens"] == 0) & (np.diff(c["lab_ptr"]) == 0)
    assert empty.sum() > 30 and not score[empty].any()  # no frame and no label: score 0


def test_one_path_and_one_frame_short(fa):
    c = case(65, "middle", "n1")
    state, seg, score, _ = run(fa, c)
    u = len(c["score"]) - 6  # (65, 33 equal labels), an empty one, (64, the same labels), an empty one, (0, one label)
    assert c["lens"][u] == 65 and c["lens"][u + 2] == 64 and len(c["labs"][u]) == 33
    a, b = int(c["ptr"][u]), int(c["ptr"][u + 1])
    assert state[a:b].tolist() == list(range(1, 66))
    la = int(c["lab_ptr"][u])
    assert seg[2 * la:2 * la + 66].tolist() == [t for i in range(33) for t in (2 * i, 2 * i)]
    for v in (u + 2, u + 4):
        assert score[v] == NEG and (state[int(c["ptr"][v]):int(c["ptr"][v + 1])] == -1).all()
        assert (seg[2 * int(c["lab_ptr"][v]):2 * int(c["lab_ptr"][v + 1])] == -1).all()
    h = case(65, "hmm", "n1")
    state, seg, score, _ = run(fa, h)
    u = len(h["score"]) - 10  # (64, 64 labels), (63, 64 labels), (129, 129 labels), (128, 129 labels), (0, one label), empty between
    assert h["lens"][u] == 64 and len(h["labs"][u]) == 64 and h["lens"][u + 2] == 63
    assert state[int(h["ptr"][u]):int(h["ptr"][u + 1])].tolist() == list(range(64)) and score[u + 2] == NEG and score[u + 6] == NEG
    assert state[int(h["ptr"][u + 4]):int(h["ptr"][u + 5])].tolist() == list(range(129))


def raw(z, ptr, labels, lab_ptr, cell, blank, state, seg, score, status, ws, C, ws_bytes=None):
    import hip_binding as hb

    hb._call("fhvae_fa_align", hb._p(z), z.stride(0), int(z.shape[0]), C, blank, hb._p(ptr), hb._p(labels), hb._p(lab_ptr), hb._p(cell),
             int(ptr.shape[0]) - 1, hb._p(state), hb._p(seg), hb._p(score), hb._p(status), hb._p(ws), ws.numel() if ws_bytes is None else ws_bytes)


def small(C=5, blank=2, seed=12):
    rng = np.random.default_rng(seed)
    lens, labs = [0, 9, 70, 0, 3, 30, 140], [[], [0, 1], [3, 3, 4, 0] * 8, [], [4], [1, 0, 1], [0, 1, 3, 4] * 17]
    ptr, lab_ptr = ptr_of(lens), ptr_of([len(l) for l in labs])
    z = rng.standard_normal((int(ptr[-1]), C)).astype(np.float32)
    labels = np.concatenate([np.asarray(l, dtype=np.int32) for l in labs])
    state, seg, score, status = R.batch(z, ptr, labels, lab_ptr, blank)
    return {"C": C, "blank": blank, "z": z, "ptr": ptr, "labels": labels, "lab_ptr": lab_ptr, "state": state, "seg": seg, "score": score,
            "status": status, "lens": np.asarray(lens), "labs": labs}


@pytest.mark.parametrize("blank", [2, -1])
def test_padded_rows_and_sentinels(fa, blank):
    c = small(blank=blank)
    C, N, U, NL = c["C"], c["z"].shape[0], len(c["score"]), len(c["labels"])
    base = run(fa, c)
    assert same_bits(base, oracle(c)) and base[3] == 0  # (no frame and no label is fine in either topology)
    wide = torch.full((N, 12), 777.0, dtype=torch.float32, device="cuda")
    wide[:, :C] = dev(c["z"])
    state = torch.full((N + 8,), -555, dtype=torch.int32, device="cuda")
    seg = torch.full((2 * NL + 8,), -555, dtype=torch.int32, device="cuda")
    score = torch.full((U + 2,), -555.0, dtype=torch.float64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    cell = ptr_of(fa.cells(c["ptr"], c["lab_ptr"], blank))
    ws = torch.empty(int(cell[-1]) + 256, dtype=torch.uint8, device="cuda")
    raw(wide, dev(c["ptr"]), dev(c["labels"]), dev(c["lab_ptr"]), dev(cell), blank, state, seg, score, status, ws, C)
    assert int(status.item()) == base[3]
    assert bool((wide[:, C:] == 777.0).all())  # the sentinel columns did not move
    assert bool((state[N:] == -555).all()) and bool((seg[2 * NL:] == -555).all()) and bool((score[U:] == -555.0).all())
    got = (state[:N].cpu().numpy(), seg[:2 * NL].cpu().numpy(), score[:U].cpu().numpy(), base[3])
    assert same_bits(got, base)
    # through the wrapper: a view of the wider rows is taken as it is; the workspace to the byte
    assert same_bits(run(fa, c, z=wide[:, :C]), base)
    state.fill_(-555), seg.fill_(-555), score.fill_(-555.0)
    raw(wide, dev(c["ptr"]), dev(c["labels"]), dev(c["lab_ptr"]), dev(cell), blank, state, seg, score, status, ws, C, ws_bytes=int(cell[-1]))
    assert same_bits((state[:N].cpu().numpy(), seg[:2 * NL].cpu().numpy(), score[:U].cpu().numpy(), int(status.item())), base)


@pytest.mark.parametrize("C,where", [(3, "first"), (65, "middle"), (128, "last"), (65, "hmm")])
def test_an_utterance_does_not_depend_on_its_batch(fa, C, where):
    c = case(C, where, "int")  # (integer scores: every tie rule is at work)
    full = run(fa, c)
    assert same_bits(run(fa, c), full)  # run to run
    for limit in (1, 1 << 14):  # one utterance per group, and a few per group
        assert same_bits(run(fa, c, ws_limit=limit), full), limit
    # reversed, at another leading dimension
    U = len(c["score"])
    order = list(range(U))[::-1]
    rows = np.concatenate([c["z"][c["ptr"][u]:c["ptr"][u + 1]] for u in order])
    labs = [c["labs"][u] for u in order]
    rev = {"z": rows, "ptr": ptr_of(c["lens"][order]), "labels": np.concatenate([np.asarray(l, dtype=np.int32) for l in labs]),
           "lab_ptr": ptr_of([len(l) for l in labs]), "blank": c["blank"]}
    wide = torch.zeros(rows.shape[0], C + 12 - C % 4, dtype=torch.float32, device="cuda")
    wide[:, :C] = dev(rows)
    got = run(fa, rev, z=wide[:, :C])
    assert np.array_equal(bits64(got[2]), bits64(full[2][order]))
    assert np.array_equal(got[0], np.concatenate([full[0][c["ptr"][u]:c["ptr"][u + 1]] for u in order]))
    assert np.array_equal(got[1], np.concatenate([full[1][2 * c["lab_ptr"][u]:2 * c["lab_ptr"][u + 1]] for u in order]))
    # one utterance of every kernel (1, 2, 4 and 9 states per lane) alone
    picked = {}
    for u in range(U):
        L = len(c["labs"][u])
        S = 2 * L + 1 if c["blank"] >= 0 else L
        if c["lens"][u] > 64 and np.isfinite(c["score"][u]):
            picked.setdefault(1 if S <= 64 else 2 if S <= 128 else 4 if S <= 256 else 9, u)
    assert sorted(picked) == ([1, 2, 4, 9] if c["blank"] >= 0 else [1, 2, 4])
    for u in picked.values():
        a, b = int(c["ptr"][u]), int(c["ptr"][u + 1])
        one = {"z": c["z"][a:b], "ptr": ptr_of([b - a]), "labels": np.asarray(c["labs"][u], dtype=np.int32), "lab_ptr": ptr_of([len(c["labs"][u])]),
               "blank": c["blank"]}
        got = run(fa, one)
        la, lb = 2 * int(c["lab_ptr"][u]), 2 * int(c["lab_ptr"][u + 1])
        assert bits64(got[2])[0] == bits64(full[2])[u] and np.array_equal(got[0], full[0][a:b]) and np.array_equal(got[1], full[1][la:lb]), u


def test_status_bits(fa):
    c = small()
    C, blank, U, N, NL = c["C"], c["blank"], len(c["score"]), c["z"].shape[0], len(c["labels"])
    base = run(fa, c)
    assert base[3] == 0

    def changed(u, new):
        labs = [new if v == u else l for v, l in enumerate(c["labs"])]
        return dict(c, labels=np.concatenate([np.asarray(l, dtype=np.int32) for l in labs]), lab_ptr=ptr_of([len(l) for l in labs]), labs=labs)

    def others_unchanged(d, got, u):
        for v in range(U):
            a, b = int(c["ptr"][v]), int(c["ptr"][v + 1])
            if v != u:
                assert bits64(got[2])[v] == bits64(base[2])[v] and np.array_equal(got[0][a:b], base[0][a:b]), (u, v)
                assert np.array_equal(got[1][2 * int(d["lab_ptr"][v]):2 * int(d["lab_ptr"][v + 1])],
                                      base[1][2 * int(c["lab_ptr"][v]):2 * int(c["lab_ptr"][v + 1])]), (u, v)

    # a label outside the classes, one equal to the blank, 257 labels: that utterance only
    for u, new in ((1, [0, 5]), (2, [3, blank, 4]), (4, [-1]), (5, [0, 1] * 128 + [0])):
        d = changed(u, new)
        got = run(fa, d)
        a, b = int(c["ptr"][u]), int(c["ptr"][u + 1])
        assert got[3] == fa.FA_BAD_LABEL and got[2][u] == NEG and (got[0][a:b] == -1).all(), u
        assert (got[1][2 * int(d["lab_ptr"][u]):2 * int(d["lab_ptr"][u + 1])] == -1).all() and len(new) == int(np.diff(d["lab_ptr"])[u])
        others_unchanged(d, got, u)
        want = R.batch(d["z"], d["ptr"], d["labels"], d["lab_ptr"], blank)
        assert same_bits(got, want)
    # in HMM topology class `blank` is a class like any other
    d = changed(2, [3, blank, 4])
    assert same_bits(run(fa, dict(d, blank=-1)), R.batch(d["z"], d["ptr"], d["labels"], d["lab_ptr"], -1))
    # too few frames: infeasible, that utterance only; with a refused label beside it both bits
    d = changed(4, [4, 4, 4])
    got = run(fa, d)
    assert got[3] == fa.FA_INFEASIBLE and got[2][4] == NEG and (got[0][int(c["ptr"][4]):int(c["ptr"][5])] == -1).all()
    others_unchanged(d, got, 4)
    labs = list(d["labs"])
    labs[1] = [7]
    d = dict(c, labels=np.concatenate([np.asarray(l, dtype=np.int32) for l in labs]), lab_ptr=ptr_of([len(l) for l in labs]))
    assert run(fa, d)[3] == fa.FA_INFEASIBLE | fa.FA_BAD_LABEL
    # broken pointer arrays: the bit, and nothing is written
    cell = ptr_of(fa.cells(c["ptr"], c["lab_ptr"], blank))
    ws = torch.empty(int(cell[-1]) + 256, dtype=torch.uint8, device="cuda")
    z, labels = dev(c["z"]), dev(c["labels"])
    zp = torch.nn.functional.pad(z, (0, 3))
    # sentinel-filled outputs under BAD_LABEL and INFEASIBLE together: the refused utterances hold -1 and -inf, the others their
    # values, and what lies behind the arrays does not move
    NLd = len(d["labels"])
    state = torch.full((N + 8,), -555, dtype=torch.int32, device="cuda")
    seg = torch.full((2 * NLd + 8,), -555, dtype=torch.int32, device="cuda")
    score = torch.full((U + 2,), -555.0, dtype=torch.float64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    cell_d = ptr_of(fa.cells(d["ptr"], d["lab_ptr"], blank))
    raw(zp, dev(d["ptr"]), dev(d["labels"]), dev(d["lab_ptr"]), dev(cell_d), blank, state, seg, score, status, ws, C)
    assert int(cell_d[-1]) <= ws.numel() and int(status.item()) == fa.FA_INFEASIBLE | fa.FA_BAD_LABEL
    assert bool((state[N:] == -555).all()) and bool((seg[2 * NLd:] == -555).all()) and bool((score[U:] == -555.0).all())
    assert same_bits((state[:N].cpu().numpy(), seg[:2 * NLd].cpu().numpy(), score[:U].cpu().numpy(), int(status.item())),
                     R.batch(d["z"], d["ptr"], d["labels"], d["lab_ptr"], blank))

    def broken(ptr, lab_ptr, cells, ws_bytes=None):
        state = torch.full((N,), -555, dtype=torch.int32, device="cuda")
        seg = torch.full((2 * NL + 8,), -555, dtype=torch.int32, device="cuda")
        score = torch.full((U,), -555.0, dtype=torch.float64, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        raw(zp, dev(ptr), labels, dev(lab_ptr), dev(cells), blank, state, seg, score, status, ws, C, ws_bytes)
        return int(status.item()), bool((state == -555).all()) and bool((seg == -555).all()) and bool((score == -555.0).all())

    assert broken(c["ptr"], c["lab_ptr"], cell) == (0, False)
    for i, v in ((2, 100), (0, 1), (U, N - 1), (3, -1)):
        bad = c["ptr"].copy()
        bad[i] = v
        assert broken(bad, c["lab_ptr"], cell) == (fa.FA_BAD_PTR, True), (i, v)
    for i, v in ((0, 1), (3, 1), (2, -4)):
        bad = c["lab_ptr"].copy()
        bad[i] = v
        assert broken(c["ptr"], bad, cell) == (fa.FA_BAD_PTR, True), (i, v)
    short = cell.copy()
    short[3:] -= 1  # the third utterance has one cell too few
    assert broken(c["ptr"], c["lab_ptr"], short) == (fa.FA_BAD_PTR, True)
    assert broken(c["ptr"], c["lab_ptr"], cell + 1) == (fa.FA_BAD_PTR, True)
    assert broken(c["ptr"], c["lab_ptr"], cell, ws_bytes=int(cell[-1]) - 1) == (fa.FA_BAD_PTR, True)
    assert broken(c["ptr"], c["lab_ptr"], cell, ws_bytes=int(cell[-1])) == (0, False)
    with pytest.raises(RuntimeError, match="monotone"):
        fa.align(z, dev(np.array([0, 5, 3, N, N, N, N, N])), labels, dev(c["lab_ptr"]), blank)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.align(z.cpu(), dev(c["ptr"]), labels, dev(c["lab_ptr"]), blank)
    with pytest.raises(RuntimeError, match="int32"):
        fa.align(z, dev(c["ptr"]), labels.long(), dev(c["lab_ptr"]), blank)
    with pytest.raises(RuntimeError, match="blank"):
        fa.align(z, dev(c["ptr"]), labels, dev(c["lab_ptr"]), C)


@pytest.mark.parametrize("blank", [2, -1])
def test_a_nan_row_stays_in_its_utterance(fa, blank):
    c = small(blank=blank)
    base = run(fa, c)
    z = c["z"].copy()
    z[int(c["ptr"][2]) + 17, :] = np.nan
    got = run(fa, dict(c, z=z))
    for v in range(len(c["score"])):
        a, b, la, lb = int(c["ptr"][v]), int(c["ptr"][v + 1]), 2 * int(c["lab_ptr"][v]), 2 * int(c["lab_ptr"][v + 1])
        if v != 2:
            assert bits64(got[2])[v] == bits64(base[2])[v] and np.array_equal(got[0][a:b], base[0][a:b]) and np.array_equal(got[1][la:lb], base[1][la:lb])
        else:  # unspecified, but in range
            S = 2 * len(c["labs"][2]) + 1 if blank >= 0 else len(c["labs"][2])
            assert ((got[0][a:b] >= -1) & (got[0][a:b] < S)).all() and ((got[1][la:lb] >= -1) & (got[1][la:lb] < b - a)).all()


# --------------------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def corpus():
    c = VR.corpus(60, 5, 8, 1.3, 0)
    ptr = ptr_of(c["lengths"])
    return c, ptr, int(ptr[40])


def test_align_reproduces_the_quality_figures(fa):
    """falign.align on the quality corpus of tests/test_falign_cpu.py: the oracle's bits, hence its figures."""
    import phonerec
    from test_falign_cpu import quality

    c, ptr, _ = corpus()
    lp = VR.log_posteriors(c["x"], c["means"], c["sigma"])
    labels, lab_ptr = phonerec.csr(c["refs"], "cuda")
    for z, blank in ((lp, -1), (np.concatenate([lp, np.full((lp.shape[0], 1), -3.0, np.float32)], axis=1), 5)):
        got = fa.align(dev(z), dev(ptr), labels, lab_ptr, blank)
        want = R.batch(z, ptr, labels.cpu().numpy(), lab_ptr.cpu().numpy(), blank)
        assert same_bits((got[0].cpu().numpy(), got[1].cpu().numpy().reshape(-1), got[2].cpu().numpy(), got[3]), want)
        # path_logprob: the scores are log-posteriors here, whose rows' log-sum-exp is 0 within the f32 rounding
        if blank < 0:
            lpth = fa.path_logprob(dev(z), dev(ptr), got[2]).cpu().numpy()
            assert np.allclose(lpth, want[2], rtol=0, atol=1e-4 * np.diff(ptr).max())
    hmm, near, worst, ctc_follow, unowned, argmax = quality()
    assert round(hmm, 4) == round(ctc_follow, 4) == 0.9789 and near >= 0.96


def test_fit_then_align_on_the_generators_corpus(fa, tmp_path):
    import abx
    import ctc
    import phonerec

    c, ptr, cut = corpus()
    lens = c["lengths"]
    model, hist = ctc.fit(dev(c["x"][:cut]), dev(ptr[:41]), c["refs"][:40], 5, l2=1e-4, iters=60, context=2)
    scores = fa.scores_of(dev(c["x"]), dev(ptr), model)
    assert scores.shape == (int(ptr[-1]), 6) and scores.dtype == torch.float32
    labels, lab_ptr = phonerec.csr(c["refs"], "cuda")
    state, seg, score, bits = fa.align(scores, dev(ptr), labels, lab_ptr, int(model["blank"]))
    assert bits == 0 and bool(torch.isfinite(score).all())  # every utterance is aligned
    want = R.batch(scores.cpu().numpy(), ptr, labels.cpu().numpy(), lab_ptr.cpu().numpy(), 5)
    assert same_bits((state.cpu().numpy(), seg.cpu().numpy().reshape(-1), score.cpu().numpy(), bits), want)
    st, lp = state.cpu().numpy(), lab_ptr.cpu().numpy()
    for u, ref in enumerate(c["refs"]):
        assert R.collapse(st[ptr[u]:ptr[u + 1]], ref, 5) == ref, u  # the collapsed path is the transcription
    names = ["p%d" % i for i in range(5)]
    keys = ["utt%03d" % u for u in range(60)]
    agreement = {}
    for rule in ("follow", "own"):
        sp = fa.spans(seg, lab_ptr, lens, rule)
        its = fa.items(keys, ["s1"] * 60, sp, c["refs"], names)
        path = str(tmp_path / (rule + ".item"))
        abx.write_items(path, its)
        back = abx.read_items(path)
        assert len(back) == len(sp) == int(lp[-1])
        k = ok = owned = 0
        for u, ref in enumerate(c["refs"]):
            got = np.full(int(lens[u]), -1)
            for tok in ref:
                first, count = abx.frame_range(back[k][1], back[k][2], int(lens[u]))
                assert (first, first + count - 1) == tuple(sp[k]) and back[k][0] == keys[u] and back[k][3] == names[tok]  # the items round-trip
                got[first:first + count] = tok
                k += 1
            ok += int((got == c["y"][ptr[u]:ptr[u + 1]]).sum())
            owned += int((got >= 0).sum())
        agreement[rule] = (ok / float(ptr[-1]), owned)
    # recorded, not asserted: a linear CTC model's alignments are peaky
    print("linear CTC model (context 2, 60 iterations, objective %.4f): frame agreement follow %.4f (%d frames under a token), own %.4f (%d frames)"
          % (hist["objective"][-1], agreement["follow"][0], agreement["follow"][1], agreement["own"][0], agreement["own"][1]))


# --------------------------------------------------------------------------------------------------------------------- CLI
def write_corpus(tmp_path, n_utts=12):
    """The generator's corpus as .npy files with feats.scp / len.scp, its transcriptions as Kaldi text and as an item file with the
    true times, and a frame-probe model on the true labels."""
    import abx

    c = VR.corpus(n_utts, 4, 6, 0.8, 3)
    ptr = ptr_of(c["lengths"])
    names = ["aa", "iy", "s", "sil"]
    items = []
    with open(tmp_path / "feats.scp", "w") as fs, open(tmp_path / "len.scp", "w") as ls, open(tmp_path / "text", "w") as tx:
        for u in range(n_utts):
            key = "spk%d-utt%02d" % (u % 2, u)
            np.save(tmp_path / (key + ".npy"), c["x"][ptr[u]:ptr[u + 1]])
            fs.write("%s %s\n" % (key, tmp_path / (key + ".npy")))
            ls.write("%s %d\n" % (key, c["lengths"][u]))
            tx.write(" ".join([key] + [names[p] for p in c["refs"][u]]) + "\n")
            y = c["y"][ptr[u]:ptr[u + 1]]
            edges = [0] + list(np.nonzero(np.diff(y))[0] + 1) + [len(y)]
            for i, p in enumerate(c["refs"][u]):
                items.append((key, 0.01 * edges[i], 0.01 * (edges[i + 1] - 1), names[p], "-", "-", "spk%d" % (u % 2)))
    abx.write_items(str(tmp_path / "ref.item"), items)
    (tmp_path / "phones.txt").write_text("".join(n + "\n" for n in names))
    return c, names, ["--feat-scp", str(tmp_path / "feats.scp"), "--len-scp", str(tmp_path / "len.scp"), "--on", "feats"]


def test_align_phones_cli(fa, tmp_path, capsys):
    import abx
    import align_phones as AP
    import probe

    c, names, base = write_corpus(tmp_path)
    text, item = ["--text", str(tmp_path / "text")], ["--item", str(tmp_path / "ref.item")]
    # CTC topology: fitted on the transcriptions given; --text and --item give the same aligned.item
    a, b = tmp_path / "a", tmp_path / "b"
    assert AP.main(base + text + ["--out", str(a), "--iters", "40", "--ctc-context", "1", "--spk-key-sep", "-",
                                  "--ref-item", str(tmp_path / "ref.item")]) == 0
    assert AP.main(base + item + ["--out", str(b), "--iters", "40", "--ctc-context", "1", "--spk-key-sep", "-"]) == 0
    assert sorted(p.name for p in a.iterdir()) == ["align.json", "aligned.item", "ctc.npz", "phones.txt"]
    assert (a / "aligned.item").read_bytes() == (b / "aligned.item").read_bytes() and (a / "phones.txt").read_text().split() == sorted(names)
    info = json.load(open(a / "align.json"))
    assert info["topology"] == "ctc" and info["blank_rule"] == "follow" and info["utterances"] == info["aligned"] == 12
    assert info["tokens"] == sum(len(r) for r in c["refs"]) and info["infeasible"] == [] and info["unknown"] == [] and info["context"] == 1
    assert info["mean_path_logprob_per_frame"] < 0 and "boundaries" not in json.load(open(b / "align.json"))
    rep = info["boundaries"]
    assert rep["utterances"] == 12 and rep["tokens"] == info["tokens"] and rep["skipped_sequence"] == 0 and 0 <= rep["frame_agreement"] <= 1
    got = abx.read_items(str(a / "aligned.item"))
    assert [(it[0], it[3]) for it in got] == [(it[0], it[3]) for it in abx.read_items(str(tmp_path / "ref.item"))]
    assert {it[6] for it in got} == {"spk0", "spk1"}
    # the fitted model taken again, under the own rule: another item file, the same tokens
    assert AP.main(base + text + ["--out", str(tmp_path / "own"), "--model", str(a / "ctc.npz"), "--phones", str(a / "phones.txt"),
                                  "--blank-rule", "own"]) == 0
    own = abx.read_items(str(tmp_path / "own" / "aligned.item"))
    assert [(it[0], it[3], it[1]) for it in own] == [(it[0], it[3], it[1]) for it in got] and all(o[2] <= g[2] for o, g in zip(own, got))
    assert sorted(p.name for p in (tmp_path / "own").iterdir()) == ["align.json", "aligned.item"]
    # HMM topology on a frame probe fitted on the true labels: close to the truth
    ptr = ptr_of(c["lengths"])
    pm, _ = probe.fit(dev(c["x"]), dev(c["y"]), 4, iters=30)
    probe.save(str(tmp_path / "probe.npz"), pm)
    hmm = ["--topology", "hmm", "--model", str(tmp_path / "probe.npz"), "--phones", str(tmp_path / "phones.txt"), "--ref-item", str(tmp_path / "ref.item")]
    h1, h2 = tmp_path / "h1", tmp_path / "h2"
    assert AP.main(base + text + hmm + ["--out", str(h1)]) == 0 and AP.main(base + item + hmm + ["--out", str(h2)]) == 0
    assert (h1 / "aligned.item").read_bytes() == (h2 / "aligned.item").read_bytes()
    hinfo = json.load(open(h1 / "align.json"))
    assert hinfo["topology"] == "hmm" and hinfo["aligned"] == 12 and hinfo["boundaries"]["frame_agreement"] >= 0.9
    assert hinfo["boundaries"]["within_20ms"] >= 0.9
    # an unknown utterance and an infeasible one are named, not dropped silently
    lines = (tmp_path / "text").read_text().splitlines()
    long_one = lines[1].split()[0] + " " + " ".join(["aa", "iy"] * 60)
    (tmp_path / "text2").write_text("\n".join([long_one] + lines[2:]) + "\n")
    capsys.readouterr()
    assert AP.main(base + ["--text", str(tmp_path / "text2")] + hmm + ["--out", str(tmp_path / "h3")]) == 0
    err = capsys.readouterr().err
    info3 = json.load(open(tmp_path / "h3" / "align.json"))
    assert info3["unknown"] == [lines[0].split()[0]] and info3["infeasible"] == [lines[1].split()[0]] and info3["aligned"] == 10
    assert "1 infeasible" in err and "1 unknown" in err and lines[0].split()[0] in err
    # argument checks, as recognise_phones.py
    for bad in (["--topology", "hmm"], ["--model", str(a / "ctc.npz")], ["--ctc-context", "-1"], ["--on", "z1"]):
        with pytest.raises(SystemExit):
            AP.main(base + text + ["--out", str(tmp_path / "no")] + bad)
    assert AP.main(base + ["--text", str(tmp_path / "none"), "--out", str(tmp_path / "no")]) == 1
