"""Cepstra, deltas and sliding CMVN on a MI355X (csrc/kaldi_post.hip through kaldi_post.py, prepare_kaldi_data.py,
postprocess_kaldi_feats.py and eval_model.py) against the float64 oracle of tests/kaldi_post_ref.py.

Bounds, none of them taken from the kernel's output:
  cepstra  |got - want| <= (B + 2) 2^-24 |lifter_k| sum_j |dct_kj m_j|: an f32 dot product of length B in any order (B
           roundings of partial sums, each at most 2^-24 of the sum of magnitudes, to first order) plus the two roundings of
           the scale;
  deltas   block 0 bitwise; the others (taps + 1) 2^-24 sum_j |s_j x_j|, the same argument for a chain of `taps` terms;
  CMVN     bit-equal to the oracle, which forms the same two-level float64 sums, with and without norm_vars (the device's
           float64 division and square root are correctly rounded);
  MFCC     the log-mel tolerance of tests/test_kaldi_fbank_gpu.py (4 x the float32 model's worst error against the float64
           oracle + 1e-6) carried through the DCT as lifter_k sum_j |dct_kj| tol, plus the cepstra bound; C0 with use-energy
           2^-23 |want|, the energy bound of tests/test_vad_gpu.py."""
import json
import math
import os
import zlib

import numpy as np
import pytest
import torch

import kaldi_post_ref as R
import vad_ref
from kaldi_post_ref import FB
from test_feats_cpu import _write_wav

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def KP():
    import build_ext

    build_ext.build(verbose=False)
    import kaldi_post

    kaldi_post.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return kaldi_post


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared inputs are read-only)


def ptr_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


# --------------------------------------------------------------------------------------------------------------- cepstra
@pytest.mark.parametrize("B,C", [(23, 13), (40, 40), (80, 13)])
@pytest.mark.parametrize("lifter", [False, True])
@pytest.mark.parametrize("energy", [False, True])
def test_cepstra_against_the_oracle(KP, B, C, lifter, energy):
    rng = np.random.default_rng(B * 100 + C)
    dct = KP.dct_matrix(C, B)
    lf = KP.lifter_coeffs(C, 22.0) if lifter else None
    floor = float(np.float32(math.log(50.0)))  # (the entry point takes an f32)
    for n in (1, 17, 300):  # 300 rows cross the tile of 64
        m = (rng.standard_normal((n, B + 5)) * 4.0 + 8.0).astype(np.float32)  # log-mel-like values, leading dimension B + 5
        e = (rng.standard_normal(n) * 6.0 + 4.0).astype(np.float32) if energy else None
        m_d = dev(m)[:, :B]
        assert n == 1 or m_d.stride(0) == B + 5
        got = KP.cepstra(m_d, dev(dct), dev(lf) if lifter else None, dev(e) if energy else None, floor if energy else -math.inf)
        got = got.cpu().numpy()
        want, mag = R.cepstra(m[:, :B], dct, lf, e, floor)
        assert got.shape == (n, C) and got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - want)
        bound = (B + 2) * EPS * mag
        print("cepstra B=%d C=%d n=%d: worst error / bound %.3g" % (B, C, n, (err[:, 1:] / bound[:, 1:]).max() if C > 1 else 0.0))
        assert np.all(err <= bound), (err.max(), np.unravel_index((err - bound).argmax(), err.shape))
        if energy:  # C0 is the floored energy, exactly
            assert np.array_equal(got[:, 0], np.maximum(e, np.float32(floor))) and (n == 1 or ((e < floor).any() and (e > floor).any()))
        # a row alone is bitwise the row in the batch, wherever it lies in its tile
        for f in sorted({0, n // 2, min(63, n - 1), min(64, n - 1), n - 1}):
            alone = KP.cepstra(dev(m[f:f + 1, :B]), dev(dct), dev(lf) if lifter else None, dev(e[f:f + 1]) if energy else None,
                               floor if energy else -math.inf).cpu().numpy()
            assert np.array_equal(alone[0], got[f]), (n, f)


def test_cepstra_at_the_largest_width(KP):
    """B = C = 128: the DCT matrix and the tile need more than 64 KB of LDS."""
    rng = np.random.default_rng(9)
    m = rng.standard_normal((70, 128)).astype(np.float32)
    dct = KP.dct_matrix(128, 128)
    got = KP.cepstra(dev(m), dev(dct)).cpu().numpy()
    want, mag = R.cepstra(m, dct)
    assert np.all(np.abs(got.astype(np.float64) - want) <= 130 * EPS * mag)


# ---------------------------------------------------------------------------------------------------------------- deltas
DELTA_LENS = [1, 2, 3, 0, 5, 9, 300]  # below 2 * order * window + 1 the clamps act on both sides; an empty utterance between two


@pytest.mark.parametrize("D", [13, 80])
@pytest.mark.parametrize("order,window", [(1, 2), (2, 2), (2, 3)])
def test_deltas_against_the_oracle(KP, D, order, window):
    rng = np.random.default_rng(D + 10 * order + window)
    ptr = ptr_of(DELTA_LENS)
    x = (rng.standard_normal((int(ptr[-1]), D)) * 3.0 + 1.0).astype(np.float32)
    got = KP.add_deltas(dev(x), dev(ptr), order, window).cpu().numpy()
    assert got.shape == (len(x), (order + 1) * D)
    assert np.array_equal(got[:, :D], x)  # block 0: a copy
    scales = KP.delta_scales(order, window)
    for u, T in enumerate(DELTA_LENS):
        a, e = int(ptr[u]), int(ptr[u + 1])
        if T == 0:
            continue
        want, mag = R.add_deltas(x[a:e], scales)
        err = np.abs(got[a:e].astype(np.float64) - want)
        for i in range(1, order + 1):
            blk = slice(i * D, (i + 1) * D)
            assert np.all(err[:, blk] <= (len(scales[i]) + 1) * EPS * mag[:, blk]), (u, i, err[:, blk].max())
        alone = KP.add_deltas(dev(x[a:e]), dev(ptr_of([T])), order, window).cpu().numpy()
        assert np.array_equal(alone, got[a:e]), u
    if order == 2:
        assert np.abs(got[:, D:]).max() > 0.1  # (the deltas are not all zero)


def test_deltas_do_not_cross_utterances(KP):
    lens = [7, 4, 0, 70, 3]
    ptr = ptr_of(lens)
    x = np.zeros((int(ptr[-1]), 13), dtype=np.float32)
    x[:7] = 1e30
    x[11:81] = -3e33
    got = KP.add_deltas(dev(x), dev(ptr), 2, 2).cpu().numpy()
    assert np.all(got[7:11] == 0.0) and np.all(got[81:] == 0.0)  # the utterances of zeros: deltas exactly 0
    assert np.array_equal(got[:, :13], x) and np.isfinite(got).all()
    # a constant utterance: every tap reads the same value, the chain's result is the same in every row
    assert np.all(got[:7, 13:] == got[0, 13:]) and np.all(got[11:81, 13:] == got[11, 13:])


# ---------------------------------------------------------------------------------------------------------- sliding CMVN
CMVN_LENS = [1, 2, 99, 100, 101, 299, 300, 301, 700, 5000]
CMVN_CASES = [(300, 100, True, False), (300, 100, True, True), (300, 100, False, False), (300, 100, False, True),
              (600, 100, False, False), (20000, 100, True, False), (20000, 100, True, True)]
_cmvn_data = {}


def cmvn_data(D):
    """One batch per width, shared by the cases: values with an offset and a drift, so that a window's mean matters."""
    if D not in _cmvn_data:
        rng = np.random.default_rng(D)
        ptr = ptr_of(CMVN_LENS)
        n = int(ptr[-1])
        x = (rng.standard_normal((n, D)) * np.linspace(0.5, 20.0, D) + np.linspace(-30.0, 30.0, D)
             + 5.0 * np.sin(np.arange(n) / 97.0)[:, None]).astype(np.float32)
        x.setflags(write=False)
        _cmvn_data[D] = (ptr, x)
    return _cmvn_data[D]


@pytest.mark.parametrize("D", [13, 39])
@pytest.mark.parametrize("case", CMVN_CASES, ids=lambda c: "w%d-m%d-%s-%s" % (c[0], c[1], "center" if c[2] else "causal", "vars" if c[3] else "mean"))
def test_cmvn_equals_the_oracle_bit_for_bit(KP, D, case):
    W, M, center, norm_vars = case
    ptr, x = cmvn_data(D)
    got = KP.cmvn_sliding(dev(x), dev(ptr), W, M, center, norm_vars).cpu().numpy()
    assert got.shape == x.shape and got.dtype == np.float32
    for u, T in enumerate(CMVN_LENS):
        a, e = int(ptr[u]), int(ptr[u + 1])
        want = R.cmvn_sliding(x[a:e], W, M, center, norm_vars)
        diff = got[a:e] != want
        if diff.any():
            ulp = np.abs(got[a:e].astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
            print("T=%d: %d of %d values differ, at most %.3g ulp" % (T, diff.sum(), diff.size, ulp.max()))
        assert not diff.any(), (T, np.argwhere(diff)[0])
        if W >= 2 * T and center and not norm_vars:  # per-utterance CMVN: the output's column means are 0
            assert np.abs(got[a:e].astype(np.float64).mean(axis=0)).max() <= 2.0 ** -20 * np.abs(x[a:e]).max()
        if T in (1, 301, 700):
            alone = KP.cmvn_sliding(dev(x[a:e]), dev(ptr_of([T])), W, M, center, norm_vars).cpu().numpy()
            assert np.array_equal(alone, got[a:e]), T


def test_cmvn_with_empty_utterances_and_chunk_multiples(KP):
    lens = [256, 0, 512, 0, 0, 257, 255]  # S(T) with T a multiple of the chunk is the prefix entry behind the last chunk
    ptr = ptr_of(lens)
    x = np.random.default_rng(4).standard_normal((int(ptr[-1]), 5)).astype(np.float32)
    for W, center in ((300, True), (100, False), (10000, True)):
        got = KP.cmvn_sliding(dev(x), dev(ptr), W, 50, center, True).cpu().numpy()
        for u, T in enumerate(lens):
            a, e = int(ptr[u]), int(ptr[u + 1])
            if T:
                assert np.array_equal(got[a:e], R.cmvn_sliding(x[a:e], W, 50, center, True)), (W, center, T)


def test_status_word_on_bad_pointers(KP):
    import hip_binding as hb

    lens = [300, 5, 700]
    good = ptr_of(lens)
    n, D = int(good[-1]), 13
    dec = good.copy()
    dec[2] = dec[1] - 5  # decreasing
    short = good.copy()
    short[-1] -= 1  # does not end at n
    late = good.copy()
    late[0] = 1  # does not start at 0
    x = dev(np.random.default_rng(1).standard_normal((n, D)).astype(np.float32))
    scales = dev(np.concatenate(KP.delta_scales(2, 2)))
    lib = KP.load_library()
    ws = torch.empty(int(lib.fhvae_kaldi_post_ws_bytes(n, 3, D)) // 8, dtype=torch.int64, device="cuda")
    for ptr, want in ((dec, KP.KPOST_BAD_PTR), (short, KP.KPOST_BAD_PTR), (late, KP.KPOST_BAD_PTR), (good, 0)):
        p = dev(ptr)
        for which in ("deltas", "cmvn"):
            out = torch.full((n, 3 * D if which == "deltas" else D), 12345.0, device="cuda")
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            if which == "deltas":
                hb._call("fhvae_kaldi_add_deltas", hb._p(x), hb._p(p), 3, n, D, 2, 2, hb._p(scales), hb._p(out), hb._p(status))
            else:
                hb._call("fhvae_kaldi_cmvn_sliding", hb._p(x), hb._p(p), 3, n, D, 300, 100, 1, 0, hb._p(ws), ws.numel() * 8, hb._p(out),
                         hb._p(status))
            torch.cuda.synchronize()
            assert int(status.item()) == want, (which, ptr)
            o = out.cpu().numpy()
            assert np.all(o == 12345.0) if want else not np.any(o == 12345.0)  # nothing written / everything written
        if want:
            with pytest.raises(RuntimeError, match="inconsistent frame_ptr"):
                KP.add_deltas(x, p)
            with pytest.raises(RuntimeError, match="inconsistent frame_ptr"):
                KP.cmvn_sliding(x, p)


# ------------------------------------------------------------------------------------------------------------ end to end
SECONDS = (0.3, 0.5, 1.0)


def utterances():
    sr = 16000
    return [FB.probe(sr, s + 0.01, 40 + j)[:int(s * sr)] for j, s in enumerate(SECONDS)]  # int16 scale, integer-valued


@pytest.mark.parametrize("use_energy", [False, True])
def test_mfcc_against_the_oracle(KP, use_energy):
    ys = utterances()
    opts = {"dither": 0.0, "use-energy": use_energy}
    got = KP.compute_kaldi_mfcc([(y / 32768.0).astype(np.float32) for y in ys], opts)
    dct, lf = KP.dct_matrix(13, 23), KP.lifter_coeffs(13, 22.0)
    N, S, P = FB.sizes(16000)
    for y, g in zip(ys, got):
        logmel = FB.fbank(y, n_mels=23)  # Kaldi's defaults: povey window, 23 bins, log of the power spectrum
        tol = 4.0 * np.abs(FB.fbank_f32(y, n_mels=23).astype(np.float64) - logmel).max() + 1e-6  # tests/test_kaldi_fbank_gpu.py
        e64 = vad_ref.log_energy64(y, N, S, remove_dc=True) if use_energy else None
        want, mag = R.cepstra(logmel, dct, lf, e64)
        assert g.shape == want.shape == (FB.n_frames(len(y), N, S), 13) and g.dtype == np.float32
        bound = np.abs(lf.astype(np.float64))[None, :] * np.abs(dct.astype(np.float64)).sum(axis=1)[None, :] * tol + (23 + 2) * EPS * mag
        err = np.abs(g.astype(np.float64) - want)
        first = 1 if use_energy else 0
        print("mfcc use-energy=%s, %d frames: worst error %.3g, log-mel tolerance %.3g, worst error / bound %.3g"
              % (use_energy, len(g), err[:, first:].max(), tol, (err[:, first:] / bound[:, first:]).max()))
        assert np.all(err[:, first:] <= bound[:, first:])
        if use_energy:
            assert np.all(err[:, 0] <= 2.0 ** -23 * np.abs(want[:, 0]))  # (the energy bound of tests/test_vad_gpu.py)
    # use-energy replaces C0 and nothing else; an energy floor acts on C0 alone
    if use_energy:
        plain = KP.compute_kaldi_mfcc([(y / 32768.0).astype(np.float32) for y in ys], {"dither": 0.0, "use-energy": False})
        floored = KP.compute_kaldi_mfcc([(y / 32768.0).astype(np.float32) for y in ys], dict(opts, **{"energy-floor": 1e7}))
        for g, p, f in zip(got, plain, floored):
            assert np.array_equal(g[:, 1:], p[:, 1:]) and np.array_equal(g[:, 1:], f[:, 1:])
            assert np.array_equal(f[:, 0], np.maximum(g[:, 0], np.float32(math.log(1e7))))
        assert any((g[:, 0] < math.log(1e7)).any() for g in got) and any((g[:, 0] > math.log(1e7)).any() for g in got)


@pytest.fixture()
def corpus(tmp_path):
    d = tmp_path / "data" / "train"
    d.mkdir(parents=True)
    keys, waves, lines = [], [], []
    for j, y in enumerate(utterances()):
        key = "spk%d_u%d" % (j % 2, j)
        _write_wav(d / (key + ".wav"), y.astype(np.int64)[:, None], 16000, 2)
        keys.append(key), waves.append((y / 32768.0).astype(np.float32))
        lines.append("%s %s\n" % (key, d / (key + ".wav")))
    (d / "wav.scp").write_text("".join(lines))
    mfcc = tmp_path / "mfcc.conf"
    mfcc.write_text("--dither=1\n--num-ceps=13\n--use-energy=true\n")
    return tmp_path / "data", d, keys, waves, str(mfcc)


def read_set(d):
    import kaldi_io_lite as K

    scp = [l.split(None, 1) for l in (d / "feats.scp").read_text().splitlines()]
    return [k for k, _ in scp], [K.load_mat(v) for _, v in scp], (d / "len.scp").read_text().splitlines()


def test_prepare_kaldi_data_with_mfcc_deltas_cmvn(KP, corpus):
    import kaldi_io_lite as K
    import prepare_kaldi_data as PK

    data, d, keys, waves, mfcc = corpus
    ids = [zlib.crc32(k.encode()) for k in keys]
    argv = [str(data), "--set_name", "train", "--seed", "5", "--mfcc_conf", mfcc, "--add-deltas", "--cmvn-sliding"]
    assert PK.main(argv) == 0
    got_keys, mats, lens = read_set(d)
    # the composition of the Python entry points on the same batch, bitwise
    base = KP.compute_kaldi_mfcc(waves, mfcc, seed=5, stream_ids=ids)
    ptr = ptr_of([len(b) for b in base])
    x = KP.add_deltas(dev(np.concatenate(base)), dev(ptr), 2, 2)
    x = KP.cmvn_sliding(x, dev(ptr), 300, 100, True, False).cpu().numpy()
    assert got_keys == keys and lens == ["%s %d" % (k, len(b)) for k, b in zip(keys, base)]
    for u, m in enumerate(mats):
        assert m.dtype == np.float32 and m.shape == (len(base[u]), 39) and np.array_equal(m, x[ptr[u]:ptr[u + 1]]), u
    # --vad drop: the rows a run without it writes, selected by vad.scp's decisions
    assert PK.main(argv + ["--vad", "drop"]) == 0
    drop_keys, dropped, drop_lens = read_set(d)
    vads = {l.split(None, 1)[0]: K.load_vec(l.split(None, 1)[1]) for l in (d / "vad.scp").read_text().splitlines()}
    assert list(vads) == keys and 0 < sum(int(v.sum()) for v in vads.values()) < int(ptr[-1])
    kept = [k for k in keys if vads[k].any()]
    assert drop_keys == kept and drop_lens == ["%s %d" % (k, int(vads[k].sum())) for k in kept]
    for k, m in zip(drop_keys, dropped):
        assert np.array_equal(m, mats[keys.index(k)][vads[k].astype(bool)]), k
    # the other options of the window, and a plain fbank with deltas
    assert PK.main(argv[:7] + ["--cmvn-sliding", "--cmn-window", "50", "--cmn-min-window", "10", "--no-cmn-center", "--cmn-norm-vars"]) == 0
    _, mats2, _ = read_set(d)
    y = KP.cmvn_sliding(dev(np.concatenate(base)), dev(ptr), 50, 10, False, True).cpu().numpy()
    for u, m in enumerate(mats2):
        assert m.shape[1] == 13 and np.array_equal(m, y[ptr[u]:ptr[u + 1]])


def test_prepare_kaldi_data_is_unchanged_without_the_flags(KP, corpus):
    import features as F
    import prepare_kaldi_data as PK

    data, d, keys, waves, _ = corpus
    conf = os.path.join(ROOT, "tests", "golden", "kaldi_fbank.conf")
    assert PK.main([str(data), "--set_name", "train", "--seed", "5", "--fbank_conf", conf]) == 0
    # what the parent wrote: features.compute_kaldi_fbank's matrices in kaldi_io_lite.write_ark_scp's bytes
    import kaldi_io_lite as K

    want = F.compute_kaldi_fbank(waves, conf, seed=5, stream_ids=[zlib.crc32(k.encode()) for k in keys])
    K.write_ark_scp(str(d / "want.ark"), str(d / "want.scp"), zip(keys, want))
    assert (d / "feats.ark").read_bytes() == (d / "want.ark").read_bytes()
    assert (d / "feats.scp").read_text() == (d / "want.scp").read_text().replace("want.ark", "feats.ark")
    assert (d / "len.scp").read_text() == "".join("%s %d\n" % (k, len(w)) for k, w in zip(keys, want))
    # the fbank with deltas goes through the same bank: block 0 is that matrix
    assert PK.main([str(data), "--set_name", "train", "--seed", "5", "--fbank_conf", conf, "--add-deltas", "--delta-order", "1"]) == 0
    _, mats, _ = read_set(d)
    for m, w in zip(mats, want):
        assert m.shape == (len(w), 160) and np.array_equal(m[:, :80], w)


def test_postprocess_round_trip(KP, tmp_path):
    import datasets as D
    import kaldi_io_lite as K
    import postprocess_kaldi_feats as PP

    rng = np.random.default_rng(11)
    lens = [40, 1, 333]
    mats = [rng.standard_normal((n, 16)).astype(np.float32) for n in lens]  # (a z1 archive: 16 values per frame)
    keys = ["a", "b", "c"]
    (tmp_path / "in").mkdir()
    K.write_ark_scp(str(tmp_path / "in" / "feats.ark"), str(tmp_path / "in" / "feats.scp"), zip(keys, mats))
    K.write_len_scp(tmp_path / "in" / "len.scp", zip(keys, lens))
    out = tmp_path / "out"
    assert PP.main(["--feat-scp", str(tmp_path / "in" / "feats.scp"), "--len-scp", str(tmp_path / "in" / "len.scp"), "--out", str(out),
                    "--add-deltas", "--cmvn-sliding", "--cmn-window", "100"]) == 0
    ptr = ptr_of(lens)
    want = KP.cmvn_sliding(KP.add_deltas(dev(np.concatenate(mats)), dev(ptr), 2, 2), dev(ptr), 100, 100, True, False).cpu().numpy()
    got_keys, got, got_lens = read_set(out)
    assert got_keys == keys and got_lens == ["%s %d" % kv for kv in zip(keys, lens)]
    for u, m in enumerate(got):
        assert np.array_equal(m, want[ptr[u]:ptr[u + 1]])
    ds = D.KaldiDataset(out / "feats.scp", out / "len.scp", min_len=20, mvn_path=str(tmp_path / "mvn.json"), seg_len=20, seg_shift=8)
    assert ds.num_segments > 0


def test_eval_model_with_a_baseline_archive(KP, tmp_path, capsys):
    import abx
    import eval_model as EM
    import kaldi_io_lite as K
    import units
    from test_units_gpu import tiny_corpus

    base, keys, lens = tiny_corpus(tmp_path)
    rng = np.random.default_rng(2)
    mats = [(rng.standard_normal((n, 39)) + (k[1:3] == "02")).astype(np.float32) for k, n in zip(keys, lens)]
    K.write_ark_scp(str(tmp_path / "mfcc.ark"), str(tmp_path / "mfcc.scp"), zip(keys, mats))
    item = str(tmp_path / "t.item")
    common = base + ["--max-recon", "2", "--abx-item", item, "--units", "4", "--units-item", item]
    plain, with_b = tmp_path / "plain", tmp_path / "with"
    assert EM.main(common + ["--out", str(plain)]) == 0
    assert EM.main(common + ["--out", str(with_b), "--baseline-feat-scp", str(tmp_path / "mfcc.scp")]) == 0
    s_plain, s_with = json.load(open(plain / "summary.json")), json.load(open(with_b / "summary.json"))
    new = sorted(set(p.name for p in with_b.iterdir()) - set(p.name for p in plain.iterdir()))
    assert new == ["abx_by_pair_mfcc.tsv", "units_centroids_mfcc.npy", "units_mfcc.txt"]
    for block in ("abx", "units"):
        assert set(s_with[block]) == set(s_plain[block]) | {"mfcc"}
        for k in s_plain[block]:  # z1, feats and the block's own entries: those of a run without the flag
            assert s_with[block][k] == s_plain[block][k], (block, k)
    # the entry's numbers: abx.evaluate / units.discover on the archive's rows directly
    rows = dev(np.concatenate(mats))
    tokens = abx.tokens_from_items(abx.read_items(item), keys, lens, 0.010, 0.0, max_per_cell=20)
    res = abx.evaluate(rows, tokens, "angular")
    for k, v in s_with["abx"]["mfcc"].items():
        assert v == (None if isinstance(res[k], float) and np.isnan(res[k]) else res[k]), k
    info, cent, _, seqs = units.discover(torch.nn.functional.pad(rows, (0, 9)).contiguous(), 39, keys, lens, "mfcc", k=4, iters=100, seed=0,
                                         items=abx.read_items(item), frame_shift=0.010, frame_offset=0.0)
    assert s_with["units"]["mfcc"] == json.loads(json.dumps(info))
    assert np.array_equal(np.load(with_b / "units_centroids_mfcc.npy"), cent) and cent.shape == (4, 39)
    got_keys, got_seqs = units.read_units(str(with_b / "units_mfcc.txt"))
    assert got_keys == keys and all(np.array_equal(a, b) for a, b in zip(got_seqs, seqs))
    # a missing key and another frame count are errors that name the key
    K.write_ark_scp(str(tmp_path / "short.ark"), str(tmp_path / "short.scp"), list(zip(keys, mats))[:-1])
    K.write_ark_scp(str(tmp_path / "cut.ark"), str(tmp_path / "cut.scp"), [(k, m[:-1] if k == keys[2] else m) for k, m in zip(keys, mats)])
    for scp, key in (("short.scp", keys[-1]), ("cut.scp", keys[2])):
        capsys.readouterr()
        assert EM.main(common + ["--out", str(tmp_path / "bad"), "--baseline-feat-scp", str(tmp_path / scp), "--baseline-name", "mfcc39"]) == 1
        assert key in capsys.readouterr().err
