"""Phone recognition on the GPU: fhvae_vit_decode and fhvae_edit_align against the scalar oracles of tests/viterbi_ref.py, bit for
bit on the same inputs (both are integer or single-rounding f32 dynamic programmes: there is no tolerance in this file); batch
independence, the status words, misuse; phonerec.recognise on the generator's corpus; recognise_phones.py and the "per" block
of eval_model.py."""
import functools
import json

import numpy as np
import pytest
import torch

import viterbi_ref as R
from trellis_cases import dev, ptr_of

pytestmark = pytest.mark.gpu

STATES = (1, 2, 3, 61, 63, 64, 65, 127, 128)
LENGTHS = (1, 2, 63, 64, 65, 300)
REF_LENS = (0, 1, 2, 63, 64, 65, 255, 256)
HYP_LENS = (0, 1, 64, 65, 257, 1000)
INF = float("inf")


@pytest.fixture(scope="module")
def pr():
    import build_ext

    build_ext.build(verbose=False)
    import phonerec

    assert torch.cuda.is_available()
    phonerec.load_library()
    return phonerec


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    return a.view(np.int32) if a.dtype == np.float32 else a


@functools.lru_cache(maxsize=None)
def vit_case(C, kind, lengths=None):
    """(emit, utt_ptr, trans, init, fin) and the oracle's (path, score) with and without fin, computed once."""
    rng = np.random.default_rng(1000 * C + len(kind))
    lens = []
    for n in (lengths or LENGTHS):  # an empty utterance before, between and after
        lens += [0, n]
    lens += [0]
    ptr = ptr_of(lens)
    N = int(ptr[-1])
    if kind == "gauss":
        emit, trans, init, fin = (rng.standard_normal(s).astype(np.float32) for s in ((N, C), (C, C), (C,), (C,)))
    else:  # integers in {-2 .. 2}: nearly every step is a tie
        emit, trans, init, fin = (rng.integers(-2, 3, s).astype(np.float32) for s in ((N, C), (C, C), (C,), (C,)))
    return emit, ptr, trans, init, fin, R.decode_batch(emit, ptr, trans, init), R.decode_batch(emit, ptr, trans, init, fin)


def run_vit(pr, emit, ptr, trans, init, fin=None):
    path, score = pr.viterbi(dev(emit), dev(ptr), dev(trans), dev(init), None if fin is None else dev(fin))
    return path.cpu().numpy(), score.cpu().numpy()


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))


# ------------------------------------------------------------------------------------------------------------------ decoder
@pytest.mark.parametrize("kind", ["gauss", "ties"])
@pytest.mark.parametrize("C", STATES)
def test_decode_against_the_oracle(pr, C, kind):
    emit, ptr, trans, init, fin, plain, with_fin = vit_case(C, kind)
    got = run_vit(pr, emit, ptr, trans, init)
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32
    assert same(got, plain), (C, kind)
    assert same(run_vit(pr, emit, ptr, trans, init, fin), with_fin), (C, kind)
    empty = np.diff(ptr) == 0
    assert empty.sum() == len(LENGTHS) + 1 and np.all(got[1][empty] == -INF)


def test_decode_a_long_utterance(pr):
    emit, ptr, trans, init, fin, plain, with_fin = vit_case(61, "gauss", (5000,))
    assert same(run_vit(pr, emit, ptr, trans, init), plain)
    assert same(run_vit(pr, emit, ptr, trans, init, fin), with_fin)


def test_left_to_right_and_all_minus_infinity(pr):
    rng = np.random.default_rng(5)
    C, lens = 7, [40, 1, 9, 3]
    ptr = ptr_of(lens)
    emit = rng.standard_normal((int(ptr[-1]), C)).astype(np.float32)
    trans = np.full((C, C), -np.inf, dtype=np.float32)
    for p in range(C):  # stay, or go one to the right
        trans[p, p] = np.log(0.6)
        if p + 1 < C:
            trans[p, p + 1] = np.log(0.4)
    init = np.full(C, -np.inf, dtype=np.float32)
    init[0] = 0.0
    fin = np.full(C, -np.inf, dtype=np.float32)
    fin[C - 1] = 0.0
    for f in (None, fin):
        want = R.decode_batch(emit, ptr, trans, init, f)
        got = run_vit(pr, emit, ptr, trans, init, f)
        assert same(got, want)
    assert np.all(np.diff(got[0][:40]) >= 0) and got[0][0] == 0 and got[0][39] == C - 1 and np.isfinite(got[1][0])
    assert got[1][1] == -INF and got[1][3] == -INF  # (too short to reach the last state) ... and still path 0
    assert not got[0][40:41].any()
    # all emissions -inf: the score is -inf and every state of the path is 0
    none = np.full_like(emit, -np.inf)
    path, score = run_vit(pr, none, ptr, np.zeros((C, C), np.float32), np.zeros(C, np.float32))
    assert not path.any() and np.all(score == -INF)
    assert same((path, score), R.decode_batch(none, ptr, np.zeros((C, C), np.float32), np.zeros(C, np.float32)))


@pytest.mark.parametrize("C", [3, 61, 65])
def test_an_utterance_does_not_depend_on_its_batch(pr, C):
    emit, ptr, trans, init, fin, plain, _ = vit_case(C, "ties")
    d_trans, d_init = dev(trans), dev(init)
    full = dev(emit)
    order = [u for u in range(len(ptr) - 1)][::-1]
    # alone, and at another leading dimension (a view of a wider array)
    wide = torch.zeros(emit.shape[0], C + 12 - C % 4, dtype=torch.float32, device="cuda")
    wide[:, :C] = full
    for u in range(len(ptr) - 1):
        a, b = int(ptr[u]), int(ptr[u + 1])
        if a == b:
            continue
        one = dev(np.array([0, b - a], dtype=np.int64))
        for rows in (full[a:b], wide[a:b, :C]):
            path, score = pr.viterbi(rows, one, d_trans, d_init)
            assert np.array_equal(path.cpu().numpy(), plain[0][a:b]) and bits(score)[0] == bits(plain[1])[u], (C, u)
    # reordered
    rows = np.concatenate([emit[ptr[u]:ptr[u + 1]] for u in order])
    got = run_vit(pr, rows, ptr_of([ptr[u + 1] - ptr[u] for u in order]), trans, init)
    assert np.array_equal(got[0], np.concatenate([plain[0][ptr[u]:ptr[u + 1]] for u in order]))
    assert np.array_equal(bits(got[1]), bits(plain[1][order]))


def test_a_nan_row_stays_in_its_utterance(pr):
    emit, ptr, trans, init, fin, plain, _ = vit_case(61, "gauss")
    bad = emit.copy()
    u = 2 * LENGTHS.index(65) + 1  # the utterance of 65 frames
    a, b = int(ptr[u]), int(ptr[u + 1])
    bad[a + 30] = np.nan
    path, score = run_vit(pr, bad, ptr, trans, init)
    assert path[a:b].min() >= 0 and path[a:b].max() < 61
    keep = np.ones(len(path), dtype=bool)
    keep[a:b] = False
    assert np.array_equal(path[keep], plain[0][keep])
    others = np.arange(len(score)) != u
    assert np.array_equal(bits(score[others]), bits(plain[1][others]))


def test_a_bad_utt_ptr_sets_the_bit_and_writes_nothing(pr):
    import hip_binding as hb

    emit, ptr, trans, init, fin, plain, _ = vit_case(3, "gauss")
    N, U = emit.shape[0], len(ptr) - 1
    e = torch.zeros(N, 4, dtype=torch.float32, device="cuda")
    e[:, :3] = dev(emit)
    ws = torch.empty(int(pr.load_library().fhvae_vit_ws_bytes(N, 3)), dtype=torch.uint8, device="cuda")
    d_trans, d_init = dev(trans), dev(init)
    for change in ("swap", "start", "end"):
        bad = ptr.copy()
        if change == "swap":
            bad[4], bad[5] = bad[5], bad[4] - 1
        elif change == "start":
            bad[0] = 1
        else:
            bad[-1] = N + 1
        path = torch.full((N,), -7, dtype=torch.int32, device="cuda")
        score = torch.full((U,), -7.0, dtype=torch.float32, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_ptr = dev(bad)
        hb._call("fhvae_vit_decode", hb._p(e), 4, N, 3, hb._p(d_trans), hb._p(d_init), None, hb._p(d_ptr), U, hb._p(path), hb._p(score),
                 hb._p(status), hb._p(ws), ws.numel())
        assert int(status.item()) == pr.VIT_BAD_PTR, change
        assert bool((path == -7).all()) and bool((score == -7.0).all()), change
        with pytest.raises(RuntimeError, match="utt_ptr"):
            pr.viterbi(dev(emit), d_ptr, d_trans, d_init)
    for call in (lambda: pr.viterbi(torch.zeros(4, 3), dev(ptr_of([4])), d_trans, d_init),
                 lambda: pr.viterbi(dev(emit).double(), dev(ptr), d_trans, d_init),
                 lambda: pr.viterbi(dev(emit), dev(ptr).int(), d_trans, d_init),
                 lambda: pr.viterbi(torch.zeros(4, 129, device="cuda"), dev(ptr_of([4])), d_trans, d_init)):
        with pytest.raises(RuntimeError):
            call()


# ------------------------------------------------------------------------------------------------------------------ aligner
@functools.lru_cache(maxsize=None)
def edit_case(alphabet):
    rng = np.random.default_rng(alphabet)
    refs, hyps = [], []
    for n in REF_LENS:
        for m in HYP_LENS:
            refs.append(rng.integers(0, alphabet, n).astype(np.int32))
            hyps.append(rng.integers(0, alphabet, m).astype(np.int32))
    for n in (1, 64, 65, 256):  # ref == hyp
        refs.append(rng.integers(0, alphabet, n).astype(np.int32))
        hyps.append(refs[-1].copy())
    refs.append((np.arange(200, dtype=np.int64) * 2 ** 23 - 2 ** 31).astype(np.int32))  # any int32 value is a token
    hyps.append(refs[-1][::2].copy())
    want = np.array([R.align_fast(r, h) for r, h in zip(refs, hyps)], dtype=np.int32)
    return refs, hyps, want


def run_align(pr, refs, hyps):
    import phonerec

    return pr.align(*phonerec.csr(refs, "cuda"), *phonerec.csr(hyps, "cuda")).cpu().numpy()


@pytest.mark.parametrize("alphabet", [2, 40])
def test_align_against_the_oracle(pr, alphabet):
    refs, hyps, want = edit_case(alphabet)
    got = run_align(pr, refs, hyps)
    assert got.dtype == np.int32 and got.shape == (len(refs), 4)
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0]
    n, m = np.array([len(r) for r in refs]), np.array([len(h) for h in hyps])
    assert np.array_equal(got[:, 0] + got[:, 1] + got[:, 3], n) and np.array_equal(got[:, 0] + got[:, 2] + got[:, 3], m)
    k = len(REF_LENS) * len(HYP_LENS)
    assert not got[k:k + 4, :3].any() and got[k:k + 4, 3].tolist() == [1, 64, 65, 256]
    assert got[-1].tolist() == [0, 100, 0, 100]
    # a pair alone, and the batch reversed
    for u in (7, 29, 41, 47):
        assert np.array_equal(run_align(pr, [refs[u]], [hyps[u]])[0], want[u]), u
    assert np.array_equal(run_align(pr, refs[::-1], hyps[::-1]), want[::-1])


def test_align_a_reference_too_long(pr):
    import hip_binding as hb
    import phonerec

    rng = np.random.default_rng(3)
    refs = [rng.integers(0, 5, n).astype(np.int32) for n in (10, 257, 256, 0)]
    hyps = [rng.integers(0, 5, n).astype(np.int32) for n in (12, 300, 200, 3)]
    with pytest.raises(RuntimeError, match="256"):
        run_align(pr, refs, hyps)
    (r, rp), (h, hp) = phonerec.csr(refs, "cuda"), phonerec.csr(hyps, "cuda")
    counts = torch.full((4, 4), -7, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    hb._call("fhvae_edit_align", hb._p(r), hb._p(rp), hb._p(h), hb._p(hp), 4, hb._p(counts), hb._p(status))
    assert int(status.item()) == pr.EDIT_BAD_REF
    got = counts.cpu().numpy()
    assert got[1].tolist() == [-1] * 4
    for u in (0, 2, 3):
        assert got[u].tolist() == list(R.align_fast(refs[u], hyps[u])), u
    # pointers that run backwards: the bit, and nothing written
    bad = rp.clone()
    bad[2] = 5
    counts.fill_(-7)
    status.zero_()
    hb._call("fhvae_edit_align", hb._p(r), hb._p(bad), hb._p(h), hb._p(hp), 4, hb._p(counts), hb._p(status))
    assert int(status.item()) & pr.EDIT_BAD_PTR and bool((counts == -7).all())
    with pytest.raises(RuntimeError, match="monotone"):
        pr.align(r, bad, h, hp)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pr.align(r.cpu(), rp, h, hp)


# --------------------------------------------------------------------------------------------------------------- end to end
def test_recognise_on_the_generators_corpus(pr):
    c = R.corpus(60, sigma=1.3, seed=0)
    ptr = ptr_of(c["lengths"])
    cut, U = int(ptr[40]), 60
    names = ["p%d" % i for i in range(5)]
    args = (dev(c["x"][:cut]), dev(c["y"][:cut]), c["lengths"][:40], dev(c["x"][cut:]), c["lengths"][40:], c["refs"][40:], names)
    model, report, hyp, ref = pr.recognise(*args, iters=50, test_y=c["y"][cut:])
    assert ref == c["refs"][40:] and len(hyp) == 20
    print("per %.4f per_argmax %.4f frame_accuracy %.4f frame_accuracy_argmax %.4f" % (
        report["per"], report["per_argmax"], report["frame_accuracy"], report["frame_accuracy_argmax"]))
    # the device's path is the oracle's on the emissions the device produced, and the counts are the oracle's
    freq = np.bincount(c["y"][:cut], minlength=5).astype(np.float64)
    emit = pr.emissions(args[3], model, freq / freq.sum())
    trans, init = pr.transitions(c["y"][:cut], c["lengths"][:40], 5)
    assert np.array_equal(bits(trans), bits(R.transitions(c["y"][:cut], c["lengths"][:40], 5)[0]))
    tptr = ptr_of(c["lengths"][40:])
    path, _ = pr.viterbi(emit, dev(tptr), dev(trans), dev(init))
    want_path, _ = R.decode_batch(emit.cpu().numpy(), tptr, trans, init)
    assert np.array_equal(path.cpu().numpy(), want_path)
    want_hyp = [R.collapse(want_path[a:b]) for a, b in zip(tptr[:-1], tptr[1:])]
    assert hyp == want_hyp
    tot = np.sum([R.align(r, h) for r, h in zip(ref, want_hyp)], axis=0)
    assert [report[k] for k in ("sub", "del", "ins", "cor")] == tot.tolist() and report["utterances"] == 20
    assert report["ref_tokens"] == sum(len(r) for r in ref) and report["per"] == (tot[0] + tot[1] + tot[2]) / report["ref_tokens"]
    assert report["per"] <= 0.5 * report["per_argmax"]
    assert report["frame_accuracy"] == float((want_path == c["y"][cut:]).mean()) and 0 < report["frame_accuracy_argmax"] <= 1
    # twice: the same bits
    model2, report2, hyp2, _ = pr.recognise(*args, iters=50, test_y=c["y"][cut:])
    assert report2 == report and hyp2 == hyp and all(np.array_equal(model[k], model2[k]) for k in model)


# --------------------------------------------------------------------------------------------------------------------- CLI
def test_recognise_phones_cli_without_a_checkpoint(pr, tmp_path, capsys):
    import recognise_phones as RP
    from test_gmm_gpu import feats_corpus

    base, keys, lens = feats_corpus(tmp_path)
    item = str(tmp_path / "t.item")
    out = tmp_path / "rec"
    common = base + ["--item", item, "--on", "feats", "--iters", "30"]
    assert RP.main(common + ["--out", str(out)]) == 0
    assert sorted(p.name for p in out.iterdir()) == ["hyp.txt", "phonerec.json", "probe.npz", "ref.txt"]
    info = json.load(open(out / "phonerec.json"))
    for key in ("on", "per", "sub", "del", "ins", "cor", "ref_tokens", "utterances", "per_argmax", "frame_accuracy", "frame_accuracy_argmax",
                "classes", "folded_classes", "smooth", "phone_penalty", "acoustic_scale", "prior_scale", "holdout", "seed"):
        assert key in info, key
    assert info["on"] == "feats" and info["classes"] == ["p0", "p1", "p2", "p3"] and info["utterances"] >= 1 and info["ref_tokens"] > 0
    assert 0.0 <= info["per"] and info["sub"] + info["del"] + info["cor"] == info["ref_tokens"]
    hyp, ref = (out / "hyp.txt").read_text().splitlines(), (out / "ref.txt").read_text().splitlines()
    assert len(hyp) == len(ref) == info["utterances"] and [l.split()[0] for l in hyp] == [l.split()[0] for l in ref]
    assert sum(len(l.split()) - 1 for l in ref) == info["ref_tokens"] and set(t for l in hyp for t in l.split()[1:]) <= set(info["classes"])
    # a phone map that folds p1 into p0 and deletes p3; the model of the first run
    (tmp_path / "map.txt").write_text("p1 p0\np3 -\n")
    folded = tmp_path / "folded"
    assert RP.main(common + ["--out", str(folded), "--probe", str(out / "probe.npz"), "--phone-map", str(tmp_path / "map.txt"),
                             "--phone-penalty", "1.5"]) == 0
    f = json.load(open(folded / "phonerec.json"))
    assert f["folded_classes"] == ["p0", "p2"] and f["phone_penalty"] == 1.5 and f["iterations"] == 0
    assert set(t for l in (folded / "ref.txt").read_text().splitlines() for t in l.split()[1:]) <= {"p0", "p2"}
    assert (folded / "probe.npz").read_bytes() == (out / "probe.npz").read_bytes()
    capsys.readouterr()
    (tmp_path / "bad.txt").write_text("p1 p0\np2\n")
    assert RP.main(common + ["--out", str(tmp_path / "no"), "--phone-map", str(tmp_path / "bad.txt")]) == 1
    assert "line 2" in capsys.readouterr().err and not (tmp_path / "no").exists()


def test_per_block_of_eval_model(pr, tmp_path):
    import eval_model as EM
    from test_units_gpu import tiny_corpus

    base, keys, lens = tiny_corpus(tmp_path)
    item = str(tmp_path / "t.item")
    common = base + ["--max-recon", "2"]
    plain, with_p = tmp_path / "plain", tmp_path / "with"
    assert EM.main(common + ["--out", str(plain)]) == 0
    assert EM.main(common + ["--out", str(with_p), "--per-item", item, "--probe-iters", "20"]) == 0
    s_plain, s_with = json.load(open(plain / "summary.json")), json.load(open(with_p / "summary.json"))
    assert sorted(p.name for p in with_p.iterdir()) == sorted(p.name for p in plain.iterdir())
    assert set(s_with) == set(s_plain) | {"per"} and "per" not in s_plain
    assert all(s_with[k] == s_plain[k] for k in ("checkpoint", "segments", "sequences"))
    assert s_with["lower_bound_per_frame"] == pytest.approx(s_plain["lower_bound_per_frame"], rel=1e-6)  # (as tests/test_units_gpu.py)
    block = s_with["per"]
    assert set(block) == {"z1", "feats", "holdout", "seed", "frame_shift", "frame_offset", "phone_penalty"} and block["holdout"] == 0.2
    for on in ("z1", "feats"):
        e = block[on]
        for key in ("per", "sub", "del", "ins", "cor", "ref_tokens", "utterances", "per_argmax", "frame_accuracy", "frame_accuracy_argmax", "classes"):
            assert key in e, (on, key)
        assert e["classes"] == ["aa", "iy", "s"] and e["ref_tokens"] > 0 and e["per"] >= 0.0
    only = tmp_path / "only"
    assert EM.main(common + ["--out", str(only), "--per-item", item, "--probe-iters", "5", "--per-on", "feats", "--per-phone-penalty", "2"]) == 0
    block = json.load(open(only / "summary.json"))["per"]
    assert "z1" not in block and "feats" in block and block["phone_penalty"] == 2.0
