"""Phone recognition without a GPU: PHONEREC_SIGNATURES against include/fhvae_viterbi.h and the built library, the entry points'
argument errors (they return before any launch), the oracles of tests/viterbi_ref.py against brute force, the host pieces of
phonerec.py (transitions, collapse, fold, read_phone_map, references, error_rate), tools/timit_items.py --tier phn-all, the
command lines' argument errors and the margin of the generator's corpus."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import viterbi_ref as R
import ext_abi
from ext_abi import aligned as _aligned, swap as _swap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, ALIGN, LIMIT = -1, -2, -4, -5


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import phonerec

    return phonerec.load_library()


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_signatures_match_the_header():
    import hip_binding as hb
    import phonerec

    text = ext_abi.header_text("fhvae_viterbi.h")
    found = ext_abi.declared("fhvae_viterbi.h", "fhvae_")
    assert found == phonerec.PHONEREC_SIGNATURES
    assert sorted(found) == ["fhvae_edit_align", "fhvae_vit_decode", "fhvae_vit_ws_bytes"]
    assert not set(found) & set(hb.SIGNATURES)
    assert int(re.search(r"#define FHVAE_VIT_MAX_STATES (\d+)", text).group(1)) == phonerec.VIT_MAX_STATES == 128
    assert int(re.search(r"#define FHVAE_EDIT_MAX_REF (\d+)", text).group(1)) == phonerec.EDIT_MAX_REF == 256
    for name, value in (("FHVAE_VIT_BAD_PTR", phonerec.VIT_BAD_PTR), ("FHVAE_EDIT_BAD_PTR", phonerec.EDIT_BAD_PTR),
                        ("FHVAE_EDIT_BAD_REF", phonerec.EDIT_BAD_REF)):
        assert int(re.search(r"%s = (\d+)" % name, text).group(1)) == value


def test_symbols_exported_and_the_main_header_untouched(lib):
    import hip_binding as hb
    import phonerec

    for name in phonerec.PHONEREC_SIGNATURES:
        assert hasattr(lib, name) and name not in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12 and len(hb.SIGNATURES) == 81  # include/fhvae_hip.h is untouched
    main = open(os.path.join(ROOT, "include", "fhvae_hip.h")).read().lower()
    assert "viterbi" not in main and "fhvae_vit" not in main and "fhvae_edit" not in main


def test_decode_errors_before_any_launch(lib):
    keep, p = _aligned()
    ws = lib.fhvae_vit_ws_bytes(10, 5)
    fn = lib.fhvae_vit_decode
    #       emit lde n_frames C trans init fin utt_ptr U path score status ws ws_bytes stream
    good = [p, 8, 10, 5, p, p, p, p, 2, p, p, p, p, ws, None]
    for i in (0, 4, 5, 7, 9, 10, 11, 12):
        assert fn(*_swap(good, i, None)) == NULL, i
    for i, bad in ((3, 0), (3, -1), (1, 4), (2, -1), (8, -1), (13, ws - 1), (13, 0)):
        assert fn(*_swap(good, i, bad)) == SHAPE, (i, bad)
    for i, bad in ((1, 6), (1, 10), (0, p + 4), (0, p + 8), (4, p + 2), (5, p + 1), (6, p + 2), (7, p + 4), (9, p + 2), (10, p + 3), (11, p + 1)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    assert fn(*_swap(_swap(good, 3, 129), 1, 132)) == LIMIT and fn(*_swap(good, 8, 1 << 31)) == LIMIT
    assert fn(*_swap(_swap(good, 3, 128), 1, 128)) == SHAPE  # (C = 128 is inside the limit: the workspace is now too small)
    # U == 0: nothing to do, whatever the data pointers are
    assert fn(None, 8, 0, 5, None, None, None, None, 0, None, None, p, None, 0, None) == 0
    del keep


def test_decode_fin_may_be_null_is_checked_without_a_launch(lib):
    # with fin NULL and everything else good the call would launch; a too-small workspace stops it after the fin check
    keep, p = _aligned()
    fn = lib.fhvae_vit_decode
    assert fn(p, 8, 10, 5, p, p, None, p, 2, p, p, p, p, 0, None) == SHAPE
    del keep


def test_align_errors_before_any_launch(lib):
    keep, p = _aligned()
    fn = lib.fhvae_edit_align
    #       ref ref_ptr hyp hyp_ptr U counts status stream
    good = [p, p, p, p, 3, p, p, None]
    for i in (0, 1, 2, 3, 5, 6):
        assert fn(*_swap(good, i, None)) == NULL, i
    assert fn(*_swap(good, 4, -1)) == SHAPE and fn(*_swap(good, 4, 1 << 31)) == LIMIT
    for i, bad in ((0, p + 2), (1, p + 4), (2, p + 1), (3, p + 4), (5, p + 2), (6, p + 2)):
        assert fn(*_swap(good, i, bad)) == ALIGN, (i, bad)
    assert fn(None, None, None, None, 0, None, p, None) == 0
    del keep


def test_workspace_is_monotone(lib):
    f = lib.fhvae_vit_ws_bytes
    for C in (1, 40, 61, 122, 128):
        last = 0
        for n in (0, 1, 2, 255, 256, 257, 1000, 360000, 3600000, 1 << 40):
            v = f(n, C)
            assert v >= last and v % 256 == 0 and v >= n * C and v < n * C + 256, (n, C)
            last = v
    assert f(0, 5) == 0 and f(1, 1) == 256 and f(256, 1) == 256 and f(257, 1) == 512 and f(1000, 61) < f(1000, 62)
    for bad in ((-1, 5), (10, 0), (10, -1), (10, 129), (1 << 62, 5)):
        assert f(*bad) == 0, bad


def test_raw_calls_refuse_before_any_c_call():
    import phonerec

    e, ptr, t, i = torch.zeros(4, 3), torch.tensor([0, 4]), torch.zeros(3, 3), torch.zeros(3)
    with pytest.raises(RuntimeError, match="viterbi.*no CPU fallback"):
        phonerec.viterbi(e, ptr, t, i)
    tok = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="align.*no CPU fallback"):
        phonerec.align(tok, torch.tensor([0, 3]), tok, torch.tensor([0, 3]))


# ------------------------------------------------------------------------------------------------------------------ oracle
def test_decode_equals_the_best_of_all_paths():
    rng = np.random.default_rng(0)
    C, T = 3, 5
    ties = 0
    for k in range(40):
        e, tr, ini, fin = (rng.integers(-2, 3, s).astype(np.float32) for s in ((T, C), (C, C), (C,), (C,)))
        f = fin if k % 2 else None
        path, score = R.decode(e, tr, ini, f)
        want_path, want_score = R.brute_force(e, tr, ini, f)  # (among equal scores: the smallest-index rule, from the end)
        assert np.array_equal(path, want_path) and float(score) == want_score, k
        scores = []
        for q in itertools.product(range(C), repeat=T):
            s = ini[q[0]] + e[0][q[0]] + sum(tr[q[t - 1]][q[t]] + e[t][q[t]] for t in range(1, T)) + (f[q[-1]] if f is not None else 0)
            scores.append(float(s))
        ties += scores.count(max(scores)) > 1
    assert ties >= 5  # the tie rule was exercised
    # forbidden transitions and the all -inf tie; an empty utterance
    e = np.zeros((4, 3), np.float32)
    tr = np.full((3, 3), -np.inf, np.float32)
    path, score = R.decode(e, tr, np.zeros(3, np.float32))
    assert not path.any() and score == -np.inf
    path, score = R.decode(np.zeros((0, 3), np.float32), tr, np.zeros(3, np.float32))
    assert path.shape == (0,) and score == -np.inf
    path, score = R.decode(e[:1], tr, np.array([0, 2, 2], np.float32))
    assert path.tolist() == [1] and score == 2.0


def test_align_against_a_plain_levenshtein():
    rng = np.random.default_rng(1)
    for k in range(200):
        n, m = rng.integers(0, 14, 2)
        alphabet = 2 if k % 2 else 5
        ref, hyp = rng.integers(0, alphabet, n), rng.integers(0, alphabet, m)
        S, D, I, Cor = R.align(ref, hyp)
        assert S + D + Cor == n and S + I + Cor == m and S + D + I == R.levenshtein(ref, hyp), (ref, hyp)
        assert R.align_fast(ref, hyp) == (S, D, I, Cor), (ref, hyp)
    assert R.align("kitten", "sitting") == R.align_fast(list(b"kitten"), list(b"sitting")) == (2, 0, 1, 4)
    assert R.align([], [1, 2]) == (0, 0, 2, 0) and R.align([1, 2, 3], []) == (0, 3, 0, 0) and R.align([5], [5]) == (0, 0, 0, 1)
    # ties go to the diagonal, then up, then left: "ab" -> "ba" is two substitutions, not a deletion and an insertion
    assert R.align([0, 1], [1, 0]) == (2, 0, 0, 0)


# ------------------------------------------------------------------------------------------------------------- host pieces
def test_transitions():
    import phonerec

    # two utterances; -1 breaks a pair; class 2 never has a successor
    labels = np.array([0, 0, 1, -1, 1, 2, 1, 1, 0], dtype=np.int32)
    lengths = [6, 3]
    # pairs: 0>0, 0>1, (1,-1: none), (-1,1: none), 1>2 | 1>1, 1>0;  firsts: 0, 1
    trans, init = phonerec.transitions(labels, lengths, 3, smooth=1.0)
    want = np.log(np.array([[2, 2, 1], [2, 2, 2], [1, 1, 1]], dtype=np.float64) / np.array([[5.0], [6.0], [3.0]]))
    assert trans.dtype == np.float32 and init.dtype == np.float32
    assert np.array_equal(trans, want.astype(np.float32)) and np.array_equal(init, np.log(np.array([2, 2, 1]) / 5.0).astype(np.float32))
    assert trans[2].tolist() == [np.float32(np.log(1 / 3.0))] * 3  # the uniform row
    ref = R.transitions(labels, lengths, 3, 1.0, 0.0)
    assert np.array_equal(trans, ref[0]) and np.array_equal(init, ref[1])
    # no smoothing: -inf where nothing was seen, the row without a count uniform; the penalty off the diagonal only
    trans0, init0 = phonerec.transitions(labels, lengths, 3, smooth=0.0, penalty=2.0)
    base = np.array([[np.log(0.5), np.log(0.5), -np.inf], [np.log(1 / 3.0)] * 3, [np.log(1 / 3.0)] * 3])
    off = 2.0 * (1 - np.eye(3))
    assert np.array_equal(trans0, (base - off).astype(np.float32)) and trans0[0][2] == -np.inf
    assert np.array_equal(init0, np.array([np.log(0.5), np.log(0.5), -np.inf], dtype=np.float32))
    ref0 = R.transitions(labels, lengths, 3, 0.0, 2.0)
    assert np.array_equal(trans0, ref0[0]) and np.array_equal(init0, ref0[1])
    # an utterance that begins unlabelled: its first LABELLED frame counts; tensors are taken too
    t2, i2 = phonerec.transitions(torch.tensor([-1, 2, 2]), torch.tensor([3]), 3, smooth=0.0)
    assert i2.tolist() == [-np.inf, -np.inf, 0.0] and t2[2].tolist() == [-np.inf, -np.inf, 0.0]
    for bad in (lambda: phonerec.transitions(labels, [5, 3], 3), lambda: phonerec.transitions(labels, lengths, 2),
                lambda: phonerec.transitions(labels, lengths, 3, smooth=-1.0)):
        with pytest.raises(ValueError):
            bad()


def test_collapse_and_fold():
    import phonerec

    path = torch.tensor([1, 1, 2, 2, 2, 1, 1, 1, 3, 0, 0], dtype=torch.int32)
    ptr = torch.tensor([0, 0, 6, 6, 8, 11], dtype=torch.int64)  # [], [1 1 2 2 2 1], [], [1 1], [3 0 0]
    tok, tp = phonerec.collapse(path, ptr)
    assert tok.dtype == torch.int32 and tp.dtype == torch.int64
    assert phonerec.uncsr(tok, tp) == [[], [1, 2, 1], [], [1], [3, 0]]
    seqs = [path[a:b].tolist() for a, b in zip(ptr[:-1], ptr[1:])]
    assert phonerec.uncsr(tok, tp) == [R.collapse(s) for s in seqs]
    # 1 -> 2 (no merging afterwards), 3 deleted
    ftok, fp = phonerec.fold(tok, tp, np.array([0, 2, 2, -1], dtype=np.int32))
    assert phonerec.uncsr(ftok, fp) == [[], [2, 2, 2], [], [2], [0]]
    with pytest.raises(ValueError, match="table"):
        phonerec.fold(tok, tp, np.array([0, 1, 2]))
    empty = phonerec.collapse(torch.zeros(0, dtype=torch.int32), torch.tensor([0, 0]))
    assert phonerec.uncsr(*empty) == [[]]
    flat, p = phonerec.csr([[1, 2], [], [3]])
    assert flat.tolist() == [1, 2, 3] and p.tolist() == [0, 2, 2, 3] and phonerec.uncsr(flat, p) == [[1, 2], [], [3]]


def test_read_phone_map(tmp_path):
    import phonerec

    names = ["aa", "ao", "q", "sil", "h#"]
    good = tmp_path / "map.txt"
    good.write_text("# 61 -> 39\nao aa\nq -\n\nh# sil\nzz yy\n")
    table, folded = phonerec.read_phone_map(str(good), names)
    assert table.dtype == np.int32 and table.tolist() == [0, 0, -1, 1, 1] and folded == ["aa", "sil"]
    (tmp_path / "short.txt").write_text("ao aa\nq\n")
    with pytest.raises(ValueError, match="short.txt line 2"):
        phonerec.read_phone_map(str(tmp_path / "short.txt"), names)
    (tmp_path / "twice.txt").write_text("ao aa\nq -\nao sil\n")
    with pytest.raises(ValueError, match="twice.txt line 3.*ao"):
        phonerec.read_phone_map(str(tmp_path / "twice.txt"), names)


def test_references_and_error_rate():
    import phonerec

    items = [("u2", 0.30, 0.40, "b", "-", "-", "s"), ("u1", 0.20, 0.30, "c", "-", "-", "s"), ("u1", 0.00, 0.001, "a", "-", "-", "s"),
             ("u9", 0.0, 0.1, "z", "-", "-", "s"), ("u1", 0.10, 0.20, "b", "-", "-", "s"), ("u2", 0.30, 0.35, "a", "-", "-", "s")]
    refs = phonerec.references(items, ["u1", "u2", "u3"])
    assert refs == [["a", "b", "c"], ["b", "a"], []]  # onset order; equal onsets in file order; a 1 ms token is still a token
    from recognise_phones import reference_ids

    names = ["b", "a"]
    assert reference_ids(refs, names) == [[1, 0, 2], [0, 1], []] and names == ["b", "a", "c"]
    r = phonerec.error_rate(np.array([[2, 0, 1, 4], [0, 3, 0, 0], [0, 0, 0, 0]]))
    assert r == {"per": 6 / 9.0, "sub": 2, "del": 3, "ins": 1, "cor": 4, "ref_tokens": 9, "utterances": 3}
    assert phonerec.error_rate(np.zeros((0, 4)))["per"] == 0.0 and phonerec.error_rate(np.array([[0, 0, 2, 0]]))["per"] == float("inf")
    assert phonerec.error_rate(torch.tensor([[1, 0, 0, 1]], dtype=torch.int32))["per"] == 0.5
    with pytest.raises(ValueError):
        phonerec.error_rate(np.array([[-1, -1, -1, -1]]))


# ------------------------------------------------------------------------------------------------------------------- tools
def test_timit_items_tier_phn_all(tmp_path):
    import importlib.util

    spec = importlib.util.spec_from_file_location("timit_items", os.path.join(ROOT, "tools", "timit_items.py"))
    TI = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(TI)
    d = tmp_path / "TRAIN" / "DR1" / "FABC0"
    d.mkdir(parents=True)
    (d / "SA1.PHN").write_text("0 1600 h#\n1600 3200 sh\n3200 4800 iy\n4800 8000 h#\n")
    (d / "SX2.PHN").write_text("0 800 q\n")
    (d / "SA1.WRD").write_text("1600 4800 she\n")
    every = TI.timit_items(str(tmp_path), 16000, "phn-all")
    assert every == [("fabc0_SA1", 0.0, 0.1, "h#", "-", "sh", "fabc0"), ("fabc0_SA1", 0.1, 0.2, "sh", "h#", "iy", "fabc0"),
                     ("fabc0_SA1", 0.2, 0.3, "iy", "sh", "h#", "fabc0"), ("fabc0_SA1", 0.3, 0.5, "h#", "iy", "-", "fabc0"),
                     ("fabc0_SX2", 0.0, 0.05, "q", "-", "-", "fabc0")]
    # the two existing tiers write what they wrote
    assert TI.timit_items(str(tmp_path), 16000, "phn") == TI.timit_items(str(tmp_path)) == [
        ("fabc0_SA1", 0.1, 0.2, "sh", "h#", "iy", "fabc0"), ("fabc0_SA1", 0.2, 0.3, "iy", "sh", "h#", "fabc0")]
    assert TI.timit_items(str(tmp_path), 16000, "wrd") == [("fabc0_SA1", 0.1, 0.3, "she", "-", "-", "fabc0")]
    out = tmp_path / "all.item"
    assert TI.main([str(tmp_path), str(out), "--tier", "phn-all"]) == 0
    import abx

    assert abx.read_items(str(out)) == every
    with pytest.raises(SystemExit):
        TI.main([str(tmp_path), str(out), "--tier", "all"])


# --------------------------------------------------------------------------------------------------------------------- CLI
def test_recognise_phones_argument_errors(tmp_path, capsys):
    import recognise_phones as RP

    base = ["--feat-scp", "f.scp", "--len-scp", "l.scp", "--item", "t.item", "--out", str(tmp_path / "o")]
    ck = ["--checkpoint", "c.tar"]
    for extra in (ck + ["--holdout", "0"], ck + ["--holdout", "1"], ck + ["--holdout", "0.2", "--test-feat-scp", "a", "--test-len-scp", "b"],
                  ck + ["--test-feat-scp", "a"], ck + ["--test-item", "x.item"], ck + ["--iters", "-1"], ck + ["--smooth", "-1"],
                  ck + ["--acoustic-scale", "0"], ck + ["--prior-scale", "-1"], ck + ["--phone-penalty", "inf"], ck + ["--frame-shift", "0"],
                  ck + ["--on", "mu2"], ["--on", "feats", "--compute-dtype", "bf16"]):
        with pytest.raises(SystemExit) as e:
            RP.parse_args(base + extra)
        assert e.value.code == 2, extra
    capsys.readouterr()
    for extra in ([], ["--on", "z1"]):
        with pytest.raises(SystemExit) as e:
            RP.parse_args(base + extra)
        err = capsys.readouterr().err
        assert e.value.code == 2 and "--checkpoint" in err and "--on" in err, extra
    with pytest.raises(SystemExit):
        RP.parse_args(base[2:] + ck)
    _, args = RP.parse_args(base + ["--on", "feats"])
    assert args.checkpoint is None and args.holdout == 0.2 and args.seed == 0 and args.l2 == 1e-4 and args.iters == 200
    assert args.acoustic_scale == 1.0 and args.prior_scale == 1.0 and args.phone_penalty == 0.0 and args.smooth == 1.0
    assert args.probe is None and args.phone_map is None and args.frame_shift == 0.010 and args.frame_offset == 0.0
    _, args = RP.parse_args(base + ck + ["--test-feat-scp", "a", "--test-len-scp", "b", "--probe", "m.npz", "--phone-penalty", "-1.5"])
    assert args.holdout is None and args.on == "z1" and args.probe == "m.npz" and args.phone_penalty == -1.5


def test_eval_model_keeps_its_defaults_and_refuses_per_item_without_data(capsys):
    import eval_model as EM

    args = EM.build_parser().parse_args(["--checkpoint", "c", "--out", "o"])
    assert args.per_item is None and args.per_on == ["z1", "feats"] and args.per_phone_map is None and args.per_phone_penalty == 0.0
    assert args.probe_item is None and args.probe_holdout == 0.2 and args.units is None and args.abx_item is None  # untouched
    base = ["--checkpoint", "c", "--out", "o"]
    data = ["--feat-scp", "f", "--len-scp", "l"]
    for extra in (["--per-item", "t.item"], data + ["--per-item", "t", "--per-on", "mu2"], data + ["--per-item", "t", "--per-phone-penalty", "nan"],
                  data + ["--baseline-feat-scp", "b.scp"]):
        with pytest.raises(SystemExit) as e:
            EM.parse_args(base + extra)
        assert e.value.code == 2, extra
    assert "--feat-scp" in capsys.readouterr().err
    args = EM.parse_args(base + data + ["--per-item", "t.item", "--baseline-feat-scp", "b.scp", "--per-on", "z1"])
    assert args.baseline_name == "mfcc" and args.per_on == ["z1"] and args.per_item == "t.item"


# ------------------------------------------------------------------------------------------------------------------ margin
def test_the_generators_corpus_separates_viterbi_from_arg_max():
    """The end-to-end corpus of tests/test_phonerec_gpu.py, with the true Gaussians' log-posteriors in place of a fitted probe
    and the oracle alone: the Viterbi pass at least halves the PER of the collapsed arg-max."""
    c = R.corpus(60, sigma=1.3, seed=0)
    assert c["x"].shape[1] == 8 and len(c["refs"]) == 60 and all(4 <= len(r) <= 8 for r in c["refs"])
    assert all(a != b for r in c["refs"] for a, b in zip(r[:-1], r[1:])) and int(c["lengths"].sum()) == c["y"].shape[0]
    ptr = np.concatenate([[0], np.cumsum(c["lengths"])])
    assert [R.collapse(c["y"][a:b]) for a, b in zip(ptr[:-1], ptr[1:])] == c["refs"]
    lp = R.log_posteriors(c["x"], c["means"], c["sigma"])
    trans, init = R.transitions(c["y"], c["lengths"], 5)
    path, _ = R.decode_batch(lp, ptr, trans, init)
    arg = lp.argmax(axis=1)
    per = R.per(c["refs"], [R.collapse(path[a:b]) for a, b in zip(ptr[:-1], ptr[1:])])
    per_argmax = R.per(c["refs"], [R.collapse(arg[a:b]) for a, b in zip(ptr[:-1], ptr[1:])])
    print("per %.4f per_argmax %.4f frame accuracy %.4f / %.4f" % (per, per_argmax, (path == c["y"]).mean(), (arg == c["y"]).mean()))
    assert per <= 0.5 * per_argmax and (path == c["y"]).mean() > (arg == c["y"]).mean()
