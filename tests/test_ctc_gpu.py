"""CTC on the GPU: fhvae_ctc_loss against the float64 oracle of tests/ctc_ref.py within the derived bounds
    |nll - oracle|     <= 4 T 2^-53 max(1, |oracle|)
    |grad - oracle64|  <= 2^-24 |oracle64| + 16 T 2^-53 max(1, |nll|)
(the first term of the second is the one rounding to f32, the rest the float64 recursion's noise); the one-path case and the
infeasible one beside it, -inf classes, padded rows with sentinel columns, grad = NULL, bitwise batch independence, repeatability
and independence of ws_limit, every status bit, a NaN row; ctc.objective, fit and recognise on the generator's corpus;
recognise_phones.py --ctc and eval_model.py --per-ctc."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import ctc_ref as R
import viterbi_ref as VR
from trellis_cases import bits32, bits64, blank_of, dev, labels_for, ptr_of

pytestmark = pytest.mark.gpu

CLASSES = (2, 3, 61, 64, 65, 128)
FRAMES = (1, 2, 63, 64, 65, 300)
LABELS = (0, 1, 2, 31, 32, 33, 127, 128, 129, 256)
EPS, F32 = 2.0 ** -53, 2.0 ** -24
INF = float("inf")


@pytest.fixture(scope="module")
def ctc():
    import build_ext

    build_ext.build(verbose=False)
    import ctc

    assert torch.cuda.is_available()
    ctc.load_library()
    return ctc


@functools.lru_cache(maxsize=None)
def case(C, where, scale):
    """One batch: every T of FRAMES (and 520) with every L of LABELS that fits, plain and with equal neighbours, an all-equal
    transcription at exactly T = 2 L - 1 and one frame short of it, empty utterances between them; the oracle's answers, once."""
    rng = np.random.default_rng(100 * C + 7 * len(where) + int(scale))
    blank = blank_of(C, where)
    shapes = []
    for T in FRAMES + (520,):
        for L in LABELS:
            for rep in (0, 2):
                lab = labels_for(rng, L, C, blank, rep)
                if (rep == 0 or L >= 3) and R.feasible(T, lab) and (T < 520 or L >= 129):
                    shapes.append((T, lab))
    same = [c for c in range(C) if c != blank][-1]
    shapes += [(65, [same] * 33), (64, [same] * 33), (0, [same])]  # one path exactly; one frame short; no frame at all
    lens, labs = [0], [[]]
    for T, lab in shapes:  # an empty utterance before, between and after
        lens += [T, 0]
        labs += [lab, []]
    ptr, lab_ptr = ptr_of(lens), ptr_of([len(l) for l in labs])
    labels = np.concatenate([np.asarray(l, dtype=np.int32) for l in labs])
    z = (scale * rng.standard_normal((int(ptr[-1]), C))).astype(np.float32)
    nll, grad, status = R.batch(z, ptr, labels, lab_ptr, blank)
    return {"C": C, "blank": blank, "z": z, "ptr": ptr, "labels": labels, "lab_ptr": lab_ptr, "nll": nll, "grad": grad, "status": status,
            "lens": np.asarray(lens), "labs": labs}


def run(ctc, c, want_grad=True, ws_limit=1 << 30, z=None):
    nll, grad, status = ctc.loss(dev(c["z"]) if z is None else z, dev(c["ptr"]), dev(c["labels"]), dev(c["lab_ptr"]), c["blank"],
                                 want_grad=want_grad, ws_limit=ws_limit)
    return nll.cpu().numpy(), (grad.cpu().numpy() if grad is not None else None), status


def shares(c, nll, grad):
    """The largest share of each bound that the differences take, over the utterances with a likelihood."""
    worst_n = worst_g = 0.0
    for u in range(len(c["ptr"]) - 1):
        a, b = int(c["ptr"][u]), int(c["ptr"][u + 1])
        want = c["nll"][u]
        if np.isinf(want):
            assert nll[u] == INF and not grad[a:b].any(), u
            continue
        T = max(b - a, 1)
        worst_n = max(worst_n, abs(nll[u] - want) / (4 * T * EPS * max(1.0, abs(want))))
        if b > a:
            bound = F32 * np.abs(c["grad"][a:b]) + 16 * T * EPS * max(1.0, abs(want))
            worst_g = max(worst_g, float((np.abs(grad[a:b].astype(np.float64) - c["grad"][a:b]) / bound).max()))
    return worst_n, worst_g


# ------------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("where,scale", [("first", 1.0), ("middle", 1.0), ("last", 1.0), ("middle", 50.0)])
@pytest.mark.parametrize("C", CLASSES)
def test_loss_against_the_oracle(ctc, C, where, scale):
    c = case(C, where, scale)
    nll, grad, status = run(ctc, c)
    assert nll.dtype == np.float64 and grad.dtype == np.float32 and grad.shape == c["z"].shape
    assert status == c["status"] == ctc.CTC_INFEASIBLE
    wn, wg = shares(c, nll, grad)
    print("C %d blank %s scale %g: %d utterances, worst share of the nll bound %.3f, of the gradient bound %.3f"
          % (C, where, scale, len(c["nll"]), wn, wg))
    assert wn <= 1.0 and wg <= 1.0
    empty = (c["lens"] == 0) & (np.diff(c["lab_ptr"]) == 0)
    assert empty.sum() > 30 and not nll[empty].any()  # no frame and no label: nll 0


def test_one_path_and_one_frame_short(ctc):
    c = case(61, "middle", 1.0)
    nll, grad, _ = run(ctc, c)
    u = len(c["nll"]) - 6  # (65, 33 equal labels), then an empty one, (64, the same labels), an empty one, (0, one label)
    assert c["lens"][u] == 65 and c["lens"][u + 2] == 64 and len(c["labs"][u]) == 33
    a, b = int(c["ptr"][u]), int(c["ptr"][u + 1])
    lp = R.log_softmax(c["z"][a:b])
    path = [c["labs"][u][0] if t % 2 == 0 else c["blank"] for t in range(65)]
    want = -sum(lp[t, k] for t, k in enumerate(path))
    assert abs(nll[u] - want) <= 4 * 65 * EPS * want
    onehot = np.exp(lp)
    onehot[np.arange(65), path] -= 1.0
    assert np.all(np.abs(grad[a:b] - onehot) <= F32 * np.abs(onehot) + 16 * 65 * EPS * want)
    for v in (u + 2, u + 4):  # one frame short; no frame
        assert nll[v] == INF and not grad[int(c["ptr"][v]):int(c["ptr"][v + 1])].any()


def test_minus_infinity_classes(ctc):
    rng = np.random.default_rng(11)
    C, blank = 7, 3
    lens, labs = [40, 40, 12], [[0, 1, 1, 2], [0, 5, 2], [6, 6]]
    ptr, lab_ptr = ptr_of(lens), ptr_of([len(l) for l in labs])
    z = rng.standard_normal((int(ptr[-1]), C)).astype(np.float32)
    z[:, 5] = -np.inf  # needed by the second utterance only
    labels = np.concatenate(labs).astype(np.int32)
    want = R.batch(z, ptr, labels, lab_ptr, blank)
    c = {"z": z, "ptr": ptr, "labels": labels, "lab_ptr": lab_ptr, "blank": blank, "nll": want[0], "grad": want[1]}
    nll, grad, status = run(ctc, c)
    assert status == want[2] == ctc.CTC_INFEASIBLE and nll[1] == INF and np.isfinite(nll[[0, 2]]).all()
    assert not grad[:, 5].any() and np.isfinite(grad).all()
    wn, wg = shares(c, nll, grad)
    assert wn <= 1.0 and wg <= 1.0


def raw(ctc, z, ptr, labels, lab_ptr, cell, blank, nll, grad, status, ws, C, ws_bytes=None):
    import hip_binding as hb

    hb._call("fhvae_ctc_loss", hb._p(z), z.stride(0), int(z.shape[0]), C, blank, hb._p(ptr), hb._p(labels), hb._p(lab_ptr),
             hb._p(cell) if cell is not None else None, int(ptr.shape[0]) - 1, hb._p(nll), hb._p(grad) if grad is not None else None,
             grad.stride(0) if grad is not None else 0, hb._p(status), hb._p(ws) if ws is not None else None,
             (ws.numel() if ws is not None else 0) if ws_bytes is None else ws_bytes)


def small(C=5, blank=2, seed=12):
    rng = np.random.default_rng(seed)
    lens, labs = [0, 9, 70, 0, 3, 30], [[], [0, 1], [3, 3, 4, 0] * 9, [], [4], [1, 0, 1]]
    ptr, lab_ptr = ptr_of(lens), ptr_of([len(l) for l in labs])
    z = rng.standard_normal((int(ptr[-1]), C)).astype(np.float32)
    labels = np.concatenate([np.asarray(l, dtype=np.int32) for l in labs])
    nll, grad, status = R.batch(z, ptr, labels, lab_ptr, blank)
    return {"C": C, "blank": blank, "z": z, "ptr": ptr, "labels": labels, "lab_ptr": lab_ptr, "nll": nll, "grad": grad, "status": status,
            "lens": np.asarray(lens), "labs": labs}


def test_padded_rows_sentinels_and_no_gradient(ctc):
    c = small()
    C, N, U = c["C"], c["z"].shape[0], len(c["nll"])
    base = run(ctc, c)
    wide = torch.full((N, 12), 777.0, dtype=torch.float32, device="cuda")
    wide[:, :C] = dev(c["z"])
    grad = torch.full((N, 16), -555.0, dtype=torch.float32, device="cuda")
    nll = torch.full((U,), -555.0, dtype=torch.float64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    cell = ptr_of(ctc.cells(c["ptr"], c["lab_ptr"]))
    ws = torch.empty(int(cell[-1]) * 8 + 256, dtype=torch.uint8, device="cuda")
    raw(ctc, wide, dev(c["ptr"]), dev(c["labels"]), dev(c["lab_ptr"]), dev(cell), c["blank"], nll, grad, status, ws, C)
    assert int(status.item()) == 0
    assert bool((wide[:, C:] == 777.0).all()) and bool((grad[:, C:] == -555.0).all())  # the sentinel columns did not move
    assert np.array_equal(bits64(nll), bits64(base[0])) and np.array_equal(bits32(grad[:, :C]), bits32(base[1]))
    # through the wrapper: a view of the wider rows is taken as it is
    again = run(ctc, c, z=wide[:, :C])
    assert np.array_equal(bits64(again[0]), bits64(base[0])) and np.array_equal(bits32(again[1]), bits32(base[1]))
    # grad = NULL: the same nll bits, with no workspace and no cell_ptr
    nll.fill_(-555.0)
    raw(ctc, wide, dev(c["ptr"]), dev(c["labels"]), dev(c["lab_ptr"]), None, c["blank"], nll, None, status, None, C)
    assert int(status.item()) == 0 and np.array_equal(bits64(nll), bits64(base[0]))
    only = run(ctc, c, want_grad=False)
    assert only[1] is None and np.array_equal(bits64(only[0]), bits64(base[0]))
    big = case(65, "last", 1.0)
    assert np.array_equal(bits64(run(ctc, big, want_grad=False)[0]), bits64(run(ctc, big)[0]))


@pytest.mark.parametrize("C,where", [(3, "first"), (61, "middle"), (128, "last")])
def test_an_utterance_does_not_depend_on_its_batch(ctc, C, where):
    c = case(C, where, 1.0)
    full = run(ctc, c)
    again = run(ctc, c)
    assert np.array_equal(bits64(full[0]), bits64(again[0])) and np.array_equal(bits32(full[1]), bits32(again[1]))  # run to run
    # the workspace limit: one utterance per group, and a few per group
    for limit in (1, 1 << 20):
        part = run(ctc, c, ws_limit=limit)
        assert part[2] == full[2] and np.array_equal(bits64(part[0]), bits64(full[0])) and np.array_equal(bits32(part[1]), bits32(full[1]))
    # reversed, at another leading dimension
    U = len(c["nll"])
    order = list(range(U))[::-1]
    rows = np.concatenate([c["z"][c["ptr"][u]:c["ptr"][u + 1]] for u in order])
    labs = [c["labs"][u] for u in order]
    rev = {"z": rows, "ptr": ptr_of(c["lens"][order]), "labels": np.concatenate([np.asarray(l, dtype=np.int32) for l in labs]),
           "lab_ptr": ptr_of([len(l) for l in labs]), "blank": c["blank"]}
    wide = torch.zeros(rows.shape[0], C + 12 - C % 4, dtype=torch.float32, device="cuda")
    wide[:, :C] = dev(rows)
    got = run(ctc, rev, z=wide[:, :C])
    assert np.array_equal(bits64(got[0]), bits64(full[0][order]))
    back = np.concatenate([full[1][c["ptr"][u]:c["ptr"][u + 1]] for u in order])
    assert np.array_equal(bits32(got[1]), bits32(back))
    # a few utterances alone (one of each kernel: 1, 2, 4 and 9 states per lane)
    picked = {}
    for u in range(U):
        L = len(c["labs"][u])
        if c["lens"][u] and np.isfinite(c["nll"][u]):
            picked.setdefault(1 if 2 * L + 1 <= 64 else 2 if 2 * L + 1 <= 128 else 4 if 2 * L + 1 <= 256 else 9, u)
    assert sorted(picked) == [1, 2, 4, 9]
    for u in picked.values():
        a, b = int(c["ptr"][u]), int(c["ptr"][u + 1])
        one = {"z": c["z"][a:b], "ptr": ptr_of([b - a]), "labels": np.asarray(c["labs"][u], dtype=np.int32), "lab_ptr": ptr_of([len(c["labs"][u])]),
               "blank": c["blank"]}
        got = run(ctc, one)
        assert bits64(got[0])[0] == bits64(full[0])[u] and np.array_equal(bits32(got[1]), bits32(full[1][a:b])), u


def test_status_bits(ctc):
    c = small()
    C, blank, U, N = c["C"], c["blank"], len(c["nll"]), c["z"].shape[0]
    base = run(ctc, c)
    assert base[2] == 0
    # a label outside the classes, one equal to the blank, 257 labels: that utterance only
    for u, new in ((1, [0, 5]), (2, [3, blank, 4]), (4, [-1]), (5, [0, 1] * 128 + [0])):
        labs = [new if v == u else l for v, l in enumerate(c["labs"])]
        d = dict(c, labels=np.concatenate([np.asarray(l, dtype=np.int32) for l in labs]), lab_ptr=ptr_of([len(l) for l in labs]))
        nll, grad, status = run(ctc, d)
        a, b = int(c["ptr"][u]), int(c["ptr"][u + 1])
        assert status == ctc.CTC_BAD_LABEL and nll[u] == INF and not grad[a:b].any(), u
        keep = np.arange(U) != u
        rows = np.ones(N, dtype=bool)
        rows[a:b] = False
        assert np.array_equal(bits64(nll[keep]), bits64(base[0][keep])) and np.array_equal(bits32(grad[rows]), bits32(base[1][rows])), u
        assert np.array_equal(nll == INF, R.batch(d["z"], d["ptr"], d["labels"], d["lab_ptr"], blank)[0] == INF)
    # too few frames: infeasible, that utterance only; with a refused label beside it both bits
    labs = [[4, 4, 4] if v == 4 else l for v, l in enumerate(c["labs"])]
    d = dict(c, labels=np.concatenate([np.asarray(l, dtype=np.int32) for l in labs]), lab_ptr=ptr_of([len(l) for l in labs]))
    nll, grad, status = run(ctc, d)
    assert status == ctc.CTC_INFEASIBLE and nll[4] == INF and np.array_equal(bits64(np.delete(nll, 4)), bits64(np.delete(base[0], 4)))
    labs[1] = [7]
    d = dict(c, labels=np.concatenate([np.asarray(l, dtype=np.int32) for l in labs]), lab_ptr=ptr_of([len(l) for l in labs]))
    assert run(ctc, d)[2] == ctc.CTC_INFEASIBLE | ctc.CTC_BAD_LABEL
    # broken pointer arrays: the bit, and nothing is written
    cell = ptr_of(ctc.cells(c["ptr"], c["lab_ptr"]))
    ws = torch.empty(int(cell[-1]) * 8 + 256, dtype=torch.uint8, device="cuda")
    z, labels = dev(c["z"]), dev(c["labels"])
    zp = torch.nn.functional.pad(z, (0, 3))

    def broken(ptr, lab_ptr, cells, ws_bytes=None, grad=True):
        nll = torch.full((U,), -555.0, dtype=torch.float64, device="cuda")
        g = torch.full((N, 8), -555.0, dtype=torch.float32, device="cuda") if grad else None
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        raw(ctc, zp, dev(ptr), labels, dev(lab_ptr), dev(cells) if grad else None, blank, nll, g, status, ws if grad else None, C, ws_bytes)
        return int(status.item()), bool((nll == -555.0).all()) and (g is None or bool((g == -555.0).all()))

    assert broken(c["ptr"], c["lab_ptr"], cell) == (0, False)
    for i, v in ((2, 100), (0, 1), (U, N - 1), (3, -1)):
        bad = c["ptr"].copy()
        bad[i] = v
        assert broken(bad, c["lab_ptr"], cell) == (ctc.CTC_BAD_PTR, True), (i, v)
        assert broken(bad, c["lab_ptr"], cell, grad=False) == (ctc.CTC_BAD_PTR, True), (i, v)
    for i, v in ((0, 1), (3, 1), (2, -4)):
        bad = c["lab_ptr"].copy()
        bad[i] = v
        assert broken(c["ptr"], bad, cell) == (ctc.CTC_BAD_PTR, True), (i, v)
    short = cell.copy()
    short[3:] -= 1  # the third utterance has one cell too few
    assert broken(c["ptr"], c["lab_ptr"], short) == (ctc.CTC_BAD_PTR, True)
    shifted = cell + 1
    assert broken(c["ptr"], c["lab_ptr"], shifted) == (ctc.CTC_BAD_PTR, True)
    assert broken(c["ptr"], c["lab_ptr"], cell, ws_bytes=int(cell[-1]) * 8 - 8) == (ctc.CTC_BAD_PTR, True)
    assert broken(c["ptr"], c["lab_ptr"], cell, ws_bytes=int(cell[-1]) * 8) == (0, False)
    with pytest.raises(RuntimeError, match="monotone"):
        ctc.loss(z, dev(np.array([0, 5, 3, N, N, N, N])), labels, dev(c["lab_ptr"]), blank)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc.loss(z.cpu(), dev(c["ptr"]), labels, dev(c["lab_ptr"]), blank)
    with pytest.raises(RuntimeError, match="int32"):
        ctc.loss(z, dev(c["ptr"]), labels.long(), dev(c["lab_ptr"]), blank)


def test_a_nan_row_stays_in_its_utterance(ctc):
    c = small()
    base = run(ctc, c)
    z = c["z"].copy()
    z[int(c["ptr"][2]) + 17, 1] = np.nan
    nll, grad, _ = run(ctc, dict(c, z=z))
    keep = np.arange(len(c["nll"])) != 2
    rows = np.ones(z.shape[0], dtype=bool)
    rows[int(c["ptr"][2]):int(c["ptr"][3])] = False
    assert np.array_equal(bits64(nll[keep]), bits64(base[0][keep])) and np.array_equal(bits32(grad[rows]), bits32(base[1][rows]))


# --------------------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def corpus():
    c = VR.corpus(60, 5, 8, 1.3, 0)
    ptr = ptr_of(c["lengths"])
    return c, ptr, int(ptr[40])


def check_objective(ctc, x, ptr, refs, params, l2, mean, std):
    """ctc.objective against the oracle on the logits the device formed, within the kernel's bounds carried through the sums."""
    import phonerec
    import probe

    N, D = x.shape
    n_classes = params.shape[0]
    blank = n_classes - 1
    labels, lab_ptr = phonerec.csr(refs, "cuda")
    value, grad = ctc.objective(dev(x), dev(ptr), labels, lab_ptr, params, l2, mean, std)
    tab, cst = probe.table(params[:, :D], params[:, D], mean, std, device="cuda")
    z = ctc.logits_of(dev(x), tab, cst, n_classes).cpu().numpy()
    want_v, want_g, nll, r = R.objective(z, x, ptr, labels.cpu().numpy(), lab_ptr.cpu().numpy(), blank, params, l2, mean, std)
    T = np.diff(ptr)
    per_utt = np.maximum(1.0, np.abs(nll))
    bound_v = float((4 * T * EPS * per_utt).sum()) / N + 8 * EPS * abs(want_v)
    assert abs(value - want_v) <= bound_v, (value, want_v, bound_v)
    # every r is within 2^-24 |r| + 16 T 2^-53 max(1, nll) of the oracle's; G sums r [x, 1] over the rows
    e = F32 * np.abs(r) + np.repeat(16 * T * EPS * per_utt, T)[:, None]
    xa = np.abs(np.concatenate([x.astype(np.float64), np.ones((N, 1))], axis=1))
    eg = e.T @ xa + 64 * EPS * (np.abs(r).T @ xa)  # (and the float64 sums' own rounding)
    bound_g = np.empty_like(params)
    bound_g[:, :D] = (eg[:, :D] + np.abs(mean)[None, :] * eg[:, D:]) / std[None, :] / N
    bound_g[:, D] = eg[:, D] / N
    assert np.all(np.abs(grad - want_g) <= bound_g + 8 * EPS * np.abs(want_g)), float(np.max(np.abs(grad - want_g) / bound_g))
    return value


def test_objective_fit_and_recognise_on_the_generators_corpus(ctc):
    import phonerec

    c, ptr, cut = corpus()
    x, refs = c["x"][:cut], c["refs"][:40]
    mean, std = x.astype(np.float64).mean(axis=0), x.astype(np.float64).std(axis=0)
    start = check_objective(ctc, x, ptr[:41], refs, np.zeros((6, 9)), 1e-4, mean, std)
    model, hist = ctc.fit(dev(x), dev(ptr[:41]), refs, 5, l2=1e-4, iters=60)
    assert hist["dropped_infeasible"] == 0 and hist["utterances"] == 40 and int(model["blank"]) == 5 and int(model["context"]) == 0
    obj = hist["objective"]
    assert obj[0] == start and all(b <= a for a, b in zip(obj[:-1], obj[1:])) and obj[-1] < obj[0]  # the history never rises
    params = np.concatenate([model["weights"], model["bias"][:, None]], axis=1)
    assert np.allclose(model["mean"], mean, rtol=1e-12) and np.allclose(model["std"], std, rtol=1e-12)
    end = check_objective(ctc, x, ptr[:41], refs, params, 1e-4, model["mean"], model["std"])
    assert end == obj[-1]
    # the same input: the same bits
    model2, hist2 = ctc.fit(dev(x), dev(ptr[:41]), refs, 5, l2=1e-4, iters=60)
    assert hist2["objective"] == obj and all(np.array_equal(model[k], model2[k]) for k in model)
    # recognise: below the collapsed arg-max of the frame probe on the same split
    names = ["p%d" % i for i in range(5)]
    lens = c["lengths"]
    _, base, _, _ = phonerec.recognise(dev(x), dev(c["y"][:cut]), lens[:40], dev(c["x"][cut:]), lens[40:], c["refs"][40:], names, iters=50)
    m0, rep0, hyp, ref = ctc.recognise(dev(x), lens[:40], refs, dev(c["x"][cut:]), lens[40:], c["refs"][40:], names, iters=60)
    assert all(np.array_equal(m0[k], model[k]) for k in model) and ref == c["refs"][40:] and len(hyp) == 20
    tok, tp = ctc.greedy(dev(c["x"][cut:]), dev(ptr_of(lens[40:])), m0)
    assert phonerec.uncsr(tok, tp) == hyp
    assert rep0["per"] == VR.per(ref, hyp) and rep0["objective"] == obj[-1] and rep0["context"] == 0
    _, rep2, _, _ = ctc.recognise(dev(x), lens[:40], refs, dev(c["x"][cut:]), lens[40:], c["refs"][40:], names, iters=60, context=2)
    print("held-out PER: CTC greedy context 0 %.4f, context 2 %.4f; frame probe arg-max %.4f, Viterbi %.4f (objective %.4f -> %.4f, %d iterations)"
          % (rep0["per"], rep2["per"], base["per_argmax"], base["per"], obj[0], obj[-1], hist["iterations"]))
    assert rep0["per"] < base["per_argmax"]
    assert rep2["context"] == 2


def test_fit_drops_and_counts_infeasible_utterances(ctc):
    c, ptr, cut = corpus()
    refs = [list(r) for r in c["refs"][:40]]
    refs[3] = [0, 1] * 45   # more labels than frames
    refs[17] = [2] * 300    # more labels than the kernel takes
    model, hist = ctc.fit(dev(c["x"][:cut]), dev(ptr[:41]), refs, 5, iters=3)
    assert hist["dropped_infeasible"] == 2 and hist["utterances"] == 38 and np.isfinite(hist["objective"]).all()
    keep = [u for u in range(40) if u not in (3, 17)]
    rows = np.concatenate([np.arange(ptr[u], ptr[u + 1]) for u in keep])
    same, hist2 = ctc.fit(dev(c["x"][rows]), dev(ptr_of(c["lengths"][keep])), [refs[u] for u in keep], 5, iters=3)
    assert hist2["objective"] == hist["objective"] and all(np.array_equal(model[k], same[k]) for k in model)
    with pytest.raises(ValueError, match="outside"):
        ctc.fit(dev(c["x"][:cut]), dev(ptr[:41]), [[5]] + refs[1:], 5)
    # from a frame-probe model: its rows are copied, the blank row starts at zero
    import probe

    pm, _ = probe.fit(dev(c["x"][:cut]), dev(c["y"][:cut]), 5, iters=20)
    warm, hw = ctc.fit(dev(c["x"][:cut]), dev(ptr[:41]), c["refs"][:40], 5, iters=0, init=pm)
    assert np.array_equal(warm["weights"][:5], pm["weights"]) and np.array_equal(warm["bias"][:5], pm["bias"])
    assert not warm["weights"][5].any() and warm["bias"][5] == 0 and np.array_equal(warm["mean"], pm["mean"]) and len(hw["objective"]) == 1


# --------------------------------------------------------------------------------------------------------------------- CLI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CTC_KEYS = {"per", "sub", "del", "ins", "cor", "objective", "iterations", "converged", "context", "dropped_infeasible"}


def same_content(got, want, path=""):
    """Two JSON values: the same keys, strings, integers and booleans; floats to 1e-6 relative (the recorded run was another
    process on another card of the same kind)."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and set(got) == set(want), path
        for k in want:
            same_content(got[k], want[k], path + "/" + k)
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), path
        for i, (g, w) in enumerate(zip(got, want)):
            same_content(g, w, "%s[%d]" % (path, i))
    elif isinstance(want, float):
        assert got == pytest.approx(want, rel=1e-6, abs=1e-9), path
    else:
        assert got == want, path


def test_recognise_phones_cli_with_ctc(ctc, tmp_path, capsys):
    import recognise_phones as RP
    from test_gmm_gpu import feats_corpus

    base, keys, lens = feats_corpus(tmp_path)
    common = base + ["--item", str(tmp_path / "t.item"), "--on", "feats", "--iters", "30"]
    plain, with_c = tmp_path / "plain", tmp_path / "ctc"
    assert RP.main(common + ["--out", str(plain)]) == 0
    # without --ctc: what the command wrote before the flag existed (recorded from the commit before it)
    info = json.load(open(plain / "phonerec.json"))
    same_content(info, json.load(open(GOLDEN + "/ctc_recognise_phones_plain.json")))
    assert (plain / "hyp.txt").read_text() == open(GOLDEN + "/ctc_recognise_phones_plain_hyp.txt").read()
    assert sorted(p.name for p in plain.iterdir()) == ["hyp.txt", "phonerec.json", "probe.npz", "ref.txt"] and "ctc" not in info
    # with --ctc: everything else byte for byte, plus ctc.npz, hyp_ctc.txt and the "ctc" block
    assert RP.main(common + ["--out", str(with_c), "--ctc"]) == 0
    assert sorted(p.name for p in with_c.iterdir()) == ["ctc.npz", "hyp.txt", "hyp_ctc.txt", "phonerec.json", "probe.npz", "ref.txt"]
    for name in ("hyp.txt", "ref.txt", "probe.npz"):
        assert (with_c / name).read_bytes() == (plain / name).read_bytes(), name
    got = json.load(open(with_c / "phonerec.json"))
    block = got.pop("ctc")
    assert got == info and CTC_KEYS <= set(block) and block["context"] == 0 and block["dropped_infeasible"] == 0 and block["init"] == "zero"
    assert block["sub"] + block["del"] + block["cor"] == block["ref_tokens"] == info["ref_tokens"] and block["iterations"] >= 1
    model = ctc.load(str(with_c / "ctc.npz"))
    assert model["weights"].shape == (5, 13) and int(model["blank"]) == 4
    hyp = (with_c / "hyp_ctc.txt").read_text().splitlines()
    assert [l.split()[0] for l in hyp] == [l.split()[0] for l in (plain / "ref.txt").read_text().splitlines()]
    assert set(t for l in hyp for t in l.split()[1:]) <= set(info["classes"])
    # spliced, and from the probe's rows
    for extra, key, value in ((["--ctc-context", "2"], "context", 2), (["--ctc-init", "probe"], "init", "probe")):
        out = tmp_path / key
        assert RP.main(common + ["--out", str(out), "--ctc"] + extra) == 0
        assert json.load(open(out / "phonerec.json"))["ctc"][key] == value
    assert ctc.load(str(tmp_path / "context" / "ctc.npz"))["weights"].shape == (5, 65)
    capsys.readouterr()
    for bad in (["--ctc-context", "1"], ["--ctc", "--ctc-context", "-1"], ["--ctc", "--ctc-init", "probe", "--ctc-context", "1"]):
        with pytest.raises(SystemExit):
            RP.main(common + ["--out", str(tmp_path / "no")] + bad)


def test_per_ctc_block_of_eval_model(ctc, tmp_path):
    import eval_model as EM
    from test_units_gpu import tiny_corpus

    base, keys, lens = tiny_corpus(tmp_path)
    common = base + ["--max-recon", "2", "--per-item", str(tmp_path / "t.item"), "--probe-iters", "20"]
    plain, with_c = tmp_path / "plain", tmp_path / "with"
    assert EM.main(common + ["--out", str(plain)]) == 0
    per = json.load(open(plain / "summary.json"))["per"]
    # recorded from the commit before the flag: the settings and the entry on the input features by content, the entry on z1 (the
    # output of an untrained network, where one rounding can move a count) by its keys
    want = json.load(open(GOLDEN + "/ctc_eval_model_per_plain.json"))
    same_content({k: v for k, v in per.items() if k != "z1"}, {k: v for k, v in want.items() if k != "z1"})
    assert set(per["z1"]) == set(want["z1"]) and per["z1"]["ref_tokens"] == want["z1"]["ref_tokens"]
    assert EM.main(common + ["--out", str(with_c), "--per-ctc", "--per-ctc-context", "1"]) == 0
    got = json.load(open(with_c / "summary.json"))["per"]
    for on in ("z1", "feats"):
        block = got[on].pop("ctc")
        assert CTC_KEYS <= set(block) and block["context"] == 1 and block["ref_tokens"] == got[on]["ref_tokens"] and block["per"] >= 0.0
    assert got == per
    with pytest.raises(SystemExit):
        EM.main(base + ["--out", str(tmp_path / "no"), "--per-ctc"])
