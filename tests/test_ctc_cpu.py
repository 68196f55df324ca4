"""CTC without a GPU: the float64 oracle of tests/ctc_ref.py against torch.nn.functional.ctc_loss (an independent implementation),
against brute-force enumeration and against finite differences; the infeasible and L = 0 rules; ctc.splice, the chain rule of
ctc.objective's host side against torch autograd, ctc.greedy on hand-written rows, save / load; CTC_SIGNATURES against
include/fhvae_ctc.h and the built library, fhvae_ctc_ws_bytes and the argument errors of fhvae_ctc_loss (they return before any
launch)."""
import os
import re

import numpy as np
import pytest
import torch

import ctc_ref as R
import ext_abi
from ext_abi import swap as _swap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, ALIGN, LIMIT = -1, -2, -4, -5
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import ctc

    return ctc.load_library()


def random_labels(rng, L, C, blank, repeats=0):
    """L labels without the blank; `repeats` of the neighbours are made equal."""
    classes = [c for c in range(C) if c != blank]
    lab = [int(rng.choice(classes))]
    for _ in range(L - 1):
        lab.append(int(rng.choice([c for c in classes if c != lab[-1]] or classes)))
    for i in rng.permutation(max(L - 1, 0))[:repeats]:
        lab[i + 1] = lab[i]
    return lab[:L]


def torch_ctc(z, labels, blank):
    """nll and d nll / d z by torch, float64 on the CPU, log_softmax inside the graph."""
    zt = torch.tensor(np.asarray(z, dtype=np.float64), requires_grad=True)
    lp = torch.log_softmax(zt, dim=1)[:, None, :]
    nll = torch.nn.functional.ctc_loss(lp, torch.tensor([labels], dtype=torch.long).reshape(1, -1), torch.tensor([z.shape[0]]),
                                       torch.tensor([len(labels)]), blank=blank, reduction="sum", zero_infinity=False)
    nll.backward()
    return float(nll.detach()), zt.grad.numpy()


# ------------------------------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("T,L,C,blank,scale", [(1, 1, 3, 0, 1.0), (5, 2, 3, 2, 1.0), (64, 20, 40, 39, 1.0), (300, 100, 62, 0, 1.0),
                                               (300, 129, 128, 64, 50.0), (520, 256, 61, 60, 1.0), (3000, 120, 40, 39, 1.0)])
def test_oracle_against_torch(T, L, C, blank, scale):
    rng = np.random.default_rng(T + L)
    z = (scale * rng.standard_normal((T, C))).astype(np.float32)
    lab = random_labels(rng, L, C, blank, repeats=min(3, T - L))
    nll, grad, flag = R.loss(z, lab, blank)
    want, wgrad = torch_ctc(z, lab, blank)
    assert flag == 0 and np.isfinite(nll)
    # two float64 recursions of T steps each: the bound the GPU test uses for the kernel
    assert abs(nll - want) <= 4 * T * EPS * max(1.0, abs(want)), (nll, want)
    assert np.abs(grad - wgrad).max() <= 16 * T * EPS * max(1.0, abs(want))
    assert R.loss(z, lab, blank, want_grad=False)[0] == nll


def test_oracle_against_brute_force():
    rng = np.random.default_rng(3)
    for T in range(1, 6):
        for C in (2, 3):
            for blank in range(C):
                classes = [c for c in range(C) if c != blank]
                for L in range(0, T + 1):
                    lab = [int(v) for v in rng.choice(classes, size=L)]
                    z = rng.standard_normal((T, C)).astype(np.float32)
                    nll, _, flag = R.loss(z, lab, blank)
                    want = R.brute_force(z, lab, blank)
                    if np.isinf(want):
                        assert np.isinf(nll) and flag == R.INFEASIBLE and not R.feasible(T, lab)
                    else:
                        assert flag == 0 and R.feasible(T, lab) and abs(nll - want) <= 1e-13 * max(1.0, want), (T, C, lab)


def test_oracle_against_finite_differences():
    rng = np.random.default_rng(4)
    T, C, blank = 7, 4, 1
    lab = [0, 2, 2, 3]
    z = rng.standard_normal((T, C))
    _, grad, _ = R.loss(z, lab, blank)
    h = 1e-5
    for t in range(T):
        for c in range(C):
            zp, zm = z.copy(), z.copy()
            zp[t, c] += h
            zm[t, c] -= h
            fd = (R.loss(zp, lab, blank)[0] - R.loss(zm, lab, blank)[0]) / (2 * h)
            assert abs(fd - grad[t, c]) <= 1e-8, (t, c)
    assert np.abs(grad.sum(axis=1)).max() <= 1e-14  # the rows of d nll / d logits sum to 0


def test_rules_of_the_header():
    rng = np.random.default_rng(5)
    z = rng.standard_normal((6, 4)).astype(np.float32)
    lp = R.log_softmax(z)
    # L = 0: the sum of -lp[blank]; the gradient is p - onehot(blank)
    nll, grad, flag = R.loss(z, [], 3)
    assert flag == 0 and abs(nll + lp[:, 3].sum()) <= 1e-14
    want = np.exp(lp)
    want[:, 3] -= 1.0
    assert np.abs(grad - want).max() <= 16 * 6 * EPS * max(1.0, nll)  # (the recursion's noise through the exponential)
    # T = L + equal neighbours: one path
    lab = [0, 0, 1, 2]  # 0 _ 0 1 2 needs 5 frames
    nll, grad, flag = R.loss(z[:5], lab, 3)
    path = [0, 3, 0, 1, 2]
    assert flag == 0 and abs(nll + sum(lp[t, c] for t, c in enumerate(path))) <= 1e-14
    want = np.exp(lp[:5])
    want[np.arange(5), path] -= 1.0
    assert np.abs(grad - want).max() <= 16 * 5 * EPS * max(1.0, nll)
    # one frame short, T = 0 with labels, a needed class at probability 0
    for rows, labels in ((z[:4], lab), (z[:0], [1])):
        nll, grad, flag = R.loss(rows, labels, 3)
        assert nll == np.inf and flag == R.INFEASIBLE and not grad.any() and grad.shape == rows.shape
    dead = z.copy()
    dead[:, 1] = -np.inf
    assert R.loss(dead, [0, 1], 3)[::2] == (np.inf, R.INFEASIBLE)
    nll, grad, flag = R.loss(dead, [0, 2], 3)  # ... and one that is not needed
    assert flag == 0 and np.isfinite(nll) and not grad[:, 1].any() and np.isfinite(grad).all()
    assert R.loss(z[:0], [], 3)[::2] == (0.0, 0)
    # labels the kernel refuses
    for labels in ([4], [-1], [3], [0] * 257):
        big = rng.standard_normal((600, 4)).astype(np.float32)
        nll, grad, flag = R.loss(big, labels, 3)
        assert nll == np.inf and flag == R.BAD_LABEL and not grad.any()


# --------------------------------------------------------------------------------------------------------------- host pieces
def test_splice():
    import ctc

    x = torch.arange(12, dtype=torch.float32).reshape(6, 2)
    ptr = torch.tensor([0, 0, 4, 5, 5, 6])
    assert ctc.splice(x, ptr, 0) is x
    got = ctc.splice(x, ptr, 1).numpy()
    rows = [[0, 0, 1], [0, 1, 2], [1, 2, 3], [2, 3, 3], [4, 4, 4], [5, 5, 5]]
    want = np.stack([np.concatenate([x[i].numpy() for i in r]) for r in rows])
    assert np.array_equal(got, want)
    got = ctc.splice(x, ptr, 2).numpy()
    assert got.shape == (6, 10) and np.array_equal(got[3], np.concatenate([x[i].numpy() for i in (1, 2, 3, 3, 3)]))
    assert ctc.splice(x[:0], torch.tensor([0, 0]), 2).shape == (0, 10)
    with pytest.raises(ValueError):
        ctc.splice(x, ptr, -1)


def test_groups_and_cells():
    import ctc

    need = ctc.cells([0, 10, 10, 40, 45], [0, 3, 3, 3, 300])
    assert need.tolist() == [70, 0, 30, 0]  # (the groups of such needs: test_hip_ext_cpu.py, test_groups_by_bytes)
    assert ctc.feasible(5, [0, 0, 1, 2]) and not ctc.feasible(4, [0, 0, 1, 2]) and ctc.feasible(0, [])


def test_objective_chain_rule_against_autograd():
    import ctc

    rng = np.random.default_rng(6)
    n_classes, D, blank, l2 = 4, 3, 3, 1e-2
    lens, refs = [6, 0, 9, 5], [[0, 1], [], [2, 2, 0], [1]]
    ptr = np.concatenate([[0], np.cumsum(lens)])
    lab_ptr = np.concatenate([[0], np.cumsum([len(r) for r in refs])])
    labels = np.concatenate([np.asarray(r, dtype=np.int64) for r in refs])
    N = int(ptr[-1])
    x = rng.standard_normal((N, D)) * 2 + 1
    mean, std = x.mean(axis=0), x.std(axis=0)
    params = rng.standard_normal((n_classes, D + 1)) * 0.3
    # torch: the objective as a function of the parameters
    pt = torch.tensor(params, requires_grad=True)
    zs = (torch.tensor(x) - torch.tensor(mean)) / torch.tensor(std)
    logits = zs @ pt[:, :D].T + pt[:, D]
    total = 0.0
    for u in range(len(lens)):
        if lens[u]:
            lp = torch.log_softmax(logits[ptr[u]:ptr[u + 1]], dim=1)[:, None, :]
            total = total + torch.nn.functional.ctc_loss(lp, torch.tensor([refs[u]]), torch.tensor([lens[u]]), torch.tensor([len(refs[u])]),
                                                         blank=blank, reduction="sum")
    value = total / N + 0.5 * l2 * (pt[:, :D] ** 2).sum()
    value.backward()
    # the oracle's objective, and ctc._host_objective on the sums G the device would form
    z64 = logits.detach().numpy()
    got_v, got_g, nll, r = R.objective(z64, x, ptr, labels, lab_ptr, blank, params, l2, mean, std)
    assert abs(got_v - float(value.detach())) <= 1e-13 and np.abs(got_g - pt.grad.numpy()).max() <= 1e-13
    G = np.concatenate([r.T @ x, r.sum(axis=0)[:, None]], axis=1)
    v2, g2 = ctc._host_objective(float(nll.sum()), float(N), G, params, l2, mean, std)
    assert abs(v2 - float(value.detach())) <= 1e-13 and np.abs(g2 - pt.grad.numpy()).max() <= 1e-12


def test_greedy_on_hand_written_rows(tmp_path):
    import ctc

    # three phones and the blank (class 3); the rows are one-hot, the model is the identity
    model = {"weights": np.eye(4), "bias": np.zeros(4), "mean": np.zeros(4), "std": np.ones(4), "classes": np.arange(4.0),
             "blank": np.float64(3), "context": np.float64(0)}
    seqs = [[3, 0, 0, 3, 0, 1, 1, 3, 3, 2], [], [3, 3], [1, 1, 1], [2, 3, 2]]
    want = [[0, 0, 1, 2], [], [], [1], [2, 2]]
    x = torch.tensor(np.eye(4, dtype=np.float32)[np.concatenate([np.asarray(s, dtype=np.int64) for s in seqs])])
    ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(s) for s in seqs])]))
    tok, tp = ctc.greedy(x, ptr, model)
    assert tok.dtype == torch.int32 and [tok[a:b].tolist() for a, b in zip(tp[:-1], tp[1:])] == want
    assert [R.collapse(s, 3) for s in seqs] == want
    # save / load keep blank and context
    path = str(tmp_path / "ctc.npz")
    ctc.save(path, model)
    back = ctc.load(path)
    assert sorted(back) == sorted(ctc.KEYS) and int(back["blank"]) == 3 and int(back["context"]) == 0
    assert np.array_equal(back["weights"], model["weights"])
    import probe

    probe.save(path, model)
    with pytest.raises(ValueError):
        ctc.load(path)


def test_loss_refuses_cpu_tensors_and_wrong_dtypes():
    import ctc

    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="device tensor"):
        ctc.loss(z, torch.tensor([0, 4]), torch.zeros(1, dtype=torch.int32), torch.tensor([0, 1]), 2)
    with pytest.raises(RuntimeError, match="device tensor"):
        ctc.fit(z, torch.tensor([0, 4]), [[0]], 2)


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_signatures_match_the_header():
    import ctc
    import hip_binding as hb

    text = ext_abi.header_text("fhvae_ctc.h")
    found = ext_abi.declared("fhvae_ctc.h", "fhvae_")
    assert found == ctc.CTC_SIGNATURES and sorted(found) == ["fhvae_ctc_loss", "fhvae_ctc_ws_bytes"]
    assert not set(found) & set(hb.SIGNATURES)
    assert int(re.search(r"#define FHVAE_CTC_MAX_CLASSES (\d+)", text).group(1)) == ctc.CTC_MAX_CLASSES == 128
    assert int(re.search(r"#define FHVAE_CTC_MAX_LABELS (\d+)", text).group(1)) == ctc.CTC_MAX_LABELS == 256
    for name, value in (("FHVAE_CTC_BAD_PTR", ctc.CTC_BAD_PTR), ("FHVAE_CTC_BAD_LABEL", ctc.CTC_BAD_LABEL), ("FHVAE_CTC_INFEASIBLE", ctc.CTC_INFEASIBLE)):
        assert int(re.search(r"%s = (\d+)" % name, text).group(1)) == value
    assert (ctc.CTC_BAD_LABEL, ctc.CTC_INFEASIBLE, ctc.CTC_MAX_LABELS) == (R.BAD_LABEL, R.INFEASIBLE, R.MAX_LABELS)


def test_symbols_exported_and_the_main_header_untouched(lib):
    import ctc
    import hip_binding as hb

    for name in ctc.CTC_SIGNATURES:
        assert hasattr(lib, name) and name not in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12 and len(hb.SIGNATURES) == 81  # include/fhvae_hip.h is untouched
    assert "ctc" not in open(os.path.join(ROOT, "include", "fhvae_hip.h")).read().lower()


def test_workspace_bytes(lib):
    f = lib.fhvae_ctc_ws_bytes
    assert f(-1) == 0 and f(0) == 0 and f((1 << 59) + 1) == 0
    last = 0
    for cells in (1, 31, 32, 33, 1000, 360000 * 201, 1 << 40, 1 << 59):
        v = f(cells)
        assert v >= last and v % 256 == 0 and 8 * cells <= v < 8 * cells + 256
        last = v


def test_loss_errors_before_any_launch(lib):
    buf = np.zeros(4096 + 16, dtype=np.uint8)  # (kept alive; the calls below return before anything would read it)
    p = (buf.ctypes.data + 15) & ~15
    fn = lib.fhvae_ctc_loss
    #       logits ldz n_frames C blank utt_ptr labels lab_ptr cell_ptr U nll grad ldg status ws ws_bytes stream
    good = [p, 8, 10, 5, 4, p, p, p, p, 2, p, p, 8, p, p, 4096, None]
    for i in (0, 5, 6, 7, 8, 10, 13, 14):
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((3, 1), (3, 0), (4, -1), (4, 5), (1, 4), (2, -1), (9, -1), (12, 4), (15, -1)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i, bad in ((1, 6), (1, 10), (12, 6), (0, p + 4), (0, p + 8), (5, p + 4), (6, p + 2), (7, p + 4), (8, p + 4), (10, p + 4), (11, p + 8),
                   (13, p + 2), (14, p + 8)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    assert fn(*_swap(_swap(_swap(good, 3, 129), 1, 132), 12, 132)) == LIMIT and fn(*_swap(good, 9, 1 << 31)) == LIMIT
    # without grad, ldg, cell_ptr, ws and ws_bytes play no part: the next refusal is the alignment of nll
    nograd = _swap(_swap(_swap(_swap(_swap(good, 11, None), 8, None), 14, None), 12, 0), 15, -1)
    assert fn(*_swap(nograd, 10, p + 4)) == ALIGN
    # U == 0: nothing to do, whatever the data pointers are
    assert fn(None, 8, 0, 5, 4, None, None, None, None, 0, None, None, 0, p, None, 0, None) == 0
    del buf
