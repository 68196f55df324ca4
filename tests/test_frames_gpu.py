"""The frame-level layer on a MI355X: fhvae_frames_gather and fhvae_frames_overlap_mean bit for bit against the numpy oracle
(frames_ref.py), the status words, encode_frames / convert_frames against model.encode / model.decode on the oracle's windows,
and extract_latents.py run as a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import frames_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1, 2, 19, 45]


@pytest.fixture(scope="module")
def hb():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding

    hip_binding.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return hip_binding


def _corpus(F, lengths=LENGTHS, seed=0):
    rng = np.random.default_rng([seed, F])
    feats = [(rng.standard_normal((n, F)) * 3 + 1).astype(np.float32) for n in lengths]
    mean = rng.standard_normal(F).astype(np.float32)
    std = rng.uniform(0.5, 2.0, F)  # float64, as the statistics files hold them
    return feats, mean, std


_POOLS = {}


def _pool(T, F, shift):
    """One resident pool per (T, F, shift) for every test of this file (the same utterances; the CSR depends on T and shift)."""
    import frames as FR

    if (T, F, shift) not in _POOLS:
        feats, mean, std = _corpus(F)
        _POOLS[(T, F, shift)] = (FR.FramePool(feats, T, shift, mean, std, device="cuda"), feats)
    return _POOLS[(T, F, shift)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _status(pool, clear=True):
    st = int(pool.status.item())
    if clear:
        pool.status.zero_()
    return st


@pytest.mark.parametrize("shift", [1, 3, 25])
@pytest.mark.parametrize("F", [80, 3])
@pytest.mark.parametrize("T", [20, 5])
def test_gather_bitwise(hb, T, F, shift):
    pool, feats = _pool(T, F, shift)
    win = pool.win_ptr_host
    assert pool.num_windows == sum(R.n_windows(n, shift) for n in LENGTHS) and pool.num_frames == sum(LENGTHS)
    inside2, inside3 = int(win[2] + (win[3] - win[2]) // 2), int(win[3] + max(1, (win[4] - win[3]) // 2))
    assert win[2] <= inside2 < win[3] < inside3 <= win[4]
    for mvn in (False, True):
        want = R.windows(feats, T, shift, pool.mean.cpu().numpy() if mvn else None, pool.inv_std.cpu().numpy() if mvn else None)
        for a, b in ((0, pool.num_windows), (inside2, inside3)):
            btf = pool.windows(a, b - a, normalise=mvn)
            tbf = pool.windows(a, b - a, time_major=True, batch_major=False, normalise=mvn)
            both = pool.windows(a, b - a, time_major=True, normalise=mvn)
            assert btf.shape == (b - a, T, F) and tbf.shape == (T, b - a, F)
            assert _same(btf, want[a:b]), (mvn, a, b)
            assert _same(tbf, np.ascontiguousarray(want[a:b].transpose(1, 0, 2)))
            assert torch.equal(both[0], btf) and torch.equal(both[1], tbf)
        # interior windows are the segments fhvae_segment_gather cuts at the same first frame
        starts, rows = [], []
        for u, n in enumerate(LENGTHS):
            for k in range(R.n_windows(n, shift)):
                if k * shift - T // 2 >= 0 and k * shift - T // 2 + T <= n:
                    starts.append(int(pool.utt_ptr_host[u]) + k * shift - T // 2), rows.append(int(win[u]) + k)
        if T == 5 and shift == 1:
            assert len(starts) == (19 - 4) + (45 - 4)
        if starts:
            seg = hb.segment_gather(pool.pool, torch.tensor(starts, device="cuda"), T, pool.mean if mvn else None, pool.inv_std if mvn else None)
            assert torch.equal(seg, pool.windows(0, pool.num_windows, normalise=mvn)[torch.tensor(rows, device="cuda")])
    assert _status(pool) == 0


@pytest.mark.parametrize("T,shift", [(20, 1), (20, 3), (20, 10), (5, 1), (5, 2)])
@pytest.mark.parametrize("F", [80, 3])
def test_overlap_mean_bitwise(hb, T, F, shift):
    import frames as FR

    pool, _ = _pool(T, F, shift)
    rng = np.random.default_rng([T, F, shift])
    seg = (rng.standard_normal((pool.num_windows, T, F)) * 2).astype(np.float32)
    seg_d = torch.from_numpy(seg).cuda()
    plan = FR.chunk_plan(LENGTHS, T, shift, 40, overlap=True)
    assert (len(plan) > 1) == (pool.num_windows > 40)
    for mvn in (False, True):
        want = R.overlap_mean(seg, LENGTHS, T, shift, pool.mean.cpu().numpy() if mvn else None, pool.std.cpu().numpy() if mvn else None)
        assert want.shape == (pool.num_frames, F)
        assert _same(pool.overlap_mean(seg_d, 0, 0, pool.num_frames, denormalise=mvn), want)
        out = torch.full((pool.num_frames, F), float("nan"), device="cuda")
        for w0, B, g0, G in plan:
            pool.overlap_mean(seg_d[w0:w0 + B], w0, g0, G, out=out[g0:g0 + G], denormalise=mvn)
        assert _same(out, want)
    assert _status(pool) == 0


def test_overlap_mean_of_windows_is_identity(hb):
    # gather then overlap mean at shift 1 on values of 19 significant bits (test_frames_cpu.test_oracle_identities: exact)
    import frames as FR

    feats, _, _ = _corpus(80)
    feats = [(f.view(np.uint32) & np.uint32(0xFFFFFFE0)).view(np.float32) for f in feats]
    pool = FR.FramePool(feats, 20, 1, device="cuda")
    got = pool.overlap_mean(pool.windows(0, pool.num_windows), 0, 0, pool.num_frames)
    assert _same(got, np.concatenate(feats)) and _status(pool) == 0


def test_status_bad_range(hb):
    import frames as FR

    T, F, shift = 20, 80, 3
    pool, _ = _pool(T, F, shift)
    rng = np.random.default_rng(7)
    seg = rng.standard_normal((pool.num_windows, T, F)).astype(np.float32)
    want = R.overlap_mean(seg, LENGTHS, T, shift)
    lo, hi = 5, pool.num_windows - 4  # the windows handed over: [lo, hi)
    utt, win = pool.utt_ptr_host, pool.win_ptr_host
    short = 0
    for u, n in enumerate(LENGTHS):
        for f in range(n):
            ks = [int(win[u]) + k for k in R.brute_covering(f, n, T, shift)]
            if ks[0] < lo or ks[-1] >= hi:
                want[utt[u] + f] = 0.0
                short += 1
    assert 0 < short < pool.num_frames
    assert _status(pool) == 0
    got = pool.overlap_mean(torch.from_numpy(seg[lo:hi]).cuda(), lo, 0, pool.num_frames, denormalise=False)
    assert _same(got, want)  # zero rows where a covering window is missing, the other rows right
    assert _status(pool) == FR.FRAMES_BAD_RANGE
    with pytest.raises(RuntimeError, match="covering window"):
        pool.status.fill_(FR.FRAMES_BAD_RANGE)
        pool.check()
    pool.status.zero_()


def test_status_bad_ptr(hb):
    import frames as FR

    T, F, shift = 5, 3, 2
    good, feats = _pool(T, F, shift)
    pool = FR.FramePool(feats, T, shift, device="cuda")
    want = R.windows(feats, T, shift)
    seg = np.random.default_rng(8).standard_normal((pool.num_windows, T, F)).astype(np.float32)
    want_om = R.overlap_mean(seg, LENGTHS, T, shift)
    # utterance 2 is given one window too many and utterance 3 one too few: both disagree with utt_ptr, utterances 0 and 1 do not
    bad = pool.win_ptr_host.copy()
    bad[3] += 1
    pool.win_ptr = torch.from_numpy(bad).cuda()
    got = pool.windows(0, pool.num_windows)
    w2 = int(bad[2])
    assert _same(got[:w2], want[:w2]) and not got[w2:].any()
    assert _status(pool) == FR.FRAMES_BAD_PTR
    got = pool.overlap_mean(torch.from_numpy(seg).cuda(), 0, 0, pool.num_frames)
    g2 = int(pool.utt_ptr_host[2])
    assert _same(got[:g2], want_om[:g2]) and not got[g2:].any()
    assert _status(pool) == FR.FRAMES_BAD_PTR
    # the last utterance is one frame longer than the pool (46 frames have the 23 windows of 45: the two CSRs agree): refused,
    # nothing is read past the pool
    pool.win_ptr = good.win_ptr
    far = pool.utt_ptr_host.copy()
    far[-1] += 1
    assert R.n_windows(46, shift) == R.n_windows(45, shift)
    pool.utt_ptr = torch.from_numpy(far).cuda()
    got = pool.windows(0, pool.num_windows)
    w3 = int(pool.win_ptr_host[3])
    assert _same(got[:w3], want[:w3]) and not got[w3:].any()
    assert _status(pool) == FR.FRAMES_BAD_PTR
    assert _status(good) == 0


def test_pool_from_kaldi_archive(hb, tmp_path):
    # compressed (CM, CM2) and plain entries of one archive: the pool holds what the host decodes, the windows follow
    import extract_latents as EL
    import frames as FR
    import kaldi_io_lite as K
    from datasets import KaldiDataset

    feats, mean, std = _corpus(80)
    keys = ["a", "b", "c", "d"]
    tok = [K.compress_mat(f, "auto") for f in feats]
    mats = [K.CompressedMatrix(t, K.header_bytes(f), p) if i != 2 else f for i, (f, (t, p)) in enumerate(zip(feats, tok))]
    EL.write_archive(str(tmp_path / "k"), keys, mats, "kaldi")
    ds = KaldiDataset(str(tmp_path / "k" / "feats.scp"), str(tmp_path / "k" / "len.scp"), 0, None, 20, 3, False)
    assert [K.read_raw(s)[0] for s in ds.seq_feats] == ["CM2", "CM2", "FM", "CM"]
    host = [ds.load_seq(i) for i in range(4)]
    pool = FR.FramePool(ds, 20, 3, mean, std, device="cuda")
    assert pool.keys == keys and list(pool.lengths) == LENGTHS
    assert _same(pool.pool, np.concatenate(host))
    assert _same(pool.windows(0, pool.num_windows), R.windows(host, 20, 3, pool.mean.cpu().numpy(), pool.inv_std.cpu().numpy()))
    assert _status(pool) == 0


# ------------------------------------------------------------------------------------------------------------ the model drivers
MT, MF, MH, MD = 20, 16, 64, 16
MLENGTHS = [1, 19, 45, 130]


def _model(kind, dtype="f32"):
    from fhvae import FHVAE
    from simple_fhvae import SimpleFHVAE

    torch.manual_seed(11)
    if kind == "fhvae":
        return FHVAE(MT * MF, [MH, MH], [MH, MH], MD, MD, [MH, MH], seg_len=MT, compute_dtype=dtype).cuda().eval()
    return SimpleFHVAE(MT * MF, [MH, MH], [MH, MH], MD, MD, [MH, MH]).cuda().eval()


_MPOOL = {}


def _mpool():
    import frames as FR

    if not _MPOOL:
        feats, mean, std = _corpus(MF, MLENGTHS, seed=3)
        pool = FR.FramePool(feats, MT, 1, mean, std, device="cuda")
        _MPOOL["p"] = (pool, R.windows(feats, MT, 1, pool.mean.cpu().numpy(), pool.inv_std.cpu().numpy()))
    return _MPOOL["p"]


def _check_encode(model, pool, win, batch):
    import frames as FR
    from utils import mu2_ratio

    x0 = torch.from_numpy(win[:batch]).cuda()
    a, b = model.encode(x0), model.encode(x0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])  # the premise: one batch twice gives the same bits
    z1, z2, mu2 = FR.encode_frames(model, pool, batch_size=batch)
    assert z1.shape == (pool.num_frames, MD) and z2.shape == (pool.num_frames, MD) and mu2.shape == (len(MLENGTHS), MD)
    plan = FR.chunk_plan(MLENGTHS, MT, 1, batch, overlap=False)
    assert len(plan) == -(-pool.num_windows // batch)
    for w0, B, _, _ in plan:
        want1, want2 = model.encode(torch.from_numpy(win[w0:w0 + B]).cuda())
        assert torch.equal(z1[w0:w0 + B], want1) and torch.equal(z2[w0:w0 + B], want2), w0
    ratio = mu2_ratio(model)
    z64, got = z2.cpu().numpy().astype(np.float64), mu2.cpu().numpy().astype(np.float64)
    for u, (lo, hi) in enumerate(zip(pool.win_ptr_host[:-1], pool.win_ptr_host[1:])):
        W = int(hi - lo)
        want = z64[lo:hi].sum(0) / (W + ratio)
        bound = W * 2.0 ** -23 * np.abs(z64[lo:hi]).sum(0) / (W + ratio)
        err = np.abs(got[u] - want)
        print("mu2 utterance %d (W = %d): max error %.3g, bound at that element %.3g" % (u, W, err.max(), bound[err.argmax()]))
        assert (err <= bound).all(), u
    return z1, z2, mu2


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_encode_frames(hb, dtype):
    pool, win = _mpool()
    _check_encode(_model("fhvae", dtype), pool, win, 64)
    assert hb.lstm_sync_status() == 0


def _ref_convert(model, pool, win, batch, target):
    """The oracle overlap mean of model.decode run on chunk_plan's chunks; target(w0, B, z2_mu) gives the chunk's z2."""
    import frames as FR

    mean, std = pool.mean.cpu().numpy(), pool.std.cpu().numpy()
    want = np.empty((pool.num_frames, pool.F), np.float32)
    plan = FR.chunk_plan(MLENGTHS, MT, 1, batch, overlap=True)
    assert len(plan) > 2
    for w0, B, g0, G in plan:
        z1, z2 = model.encode(torch.from_numpy(win[w0:w0 + B]).cuda())
        x_mu = model.decode(z1, target(w0, B, z2))[0].reshape(B, MT, MF).cpu().numpy()
        full = np.full((pool.num_windows, MT, MF), np.nan, np.float32)  # (a frame of the chunk reads the chunk's windows only)
        full[w0:w0 + B] = x_mu
        want[g0:g0 + G] = R.overlap_mean(full, MLENGTHS, MT, 1, mean, std)[g0:g0 + G]
    assert np.isfinite(want).all()
    return want


def _check_convert(model, pool, win, batch):
    import frames as FR

    U = len(MLENGTHS)
    recon = FR.convert_frames(model, pool, None, batch_size=batch)
    assert recon.shape == (pool.num_frames, MF)
    # z2=None is the window's own z2 mean
    assert _same(recon, _ref_convert(model, pool, win, batch, lambda w0, B, z2: z2))
    g = torch.Generator().manual_seed(4)
    one, per = torch.randn(MD, generator=g).cuda(), torch.randn(U, MD, generator=g).cuda()
    got_one = FR.convert_frames(model, pool, one, batch_size=batch)
    assert _same(got_one, _ref_convert(model, pool, win, batch, lambda w0, B, z2: one))
    assert torch.equal(got_one, FR.convert_frames(model, pool, one.unsqueeze(0).expand(U, -1), batch_size=batch))
    assert not torch.equal(got_one, recon)
    win_utt = pool.win_utt
    got_per = FR.convert_frames(model, pool, per, batch_size=batch)
    assert _same(got_per, _ref_convert(model, pool, win, batch, lambda w0, B, z2: per[win_utt[w0:w0 + B]]))
    with pytest.raises(ValueError, match="z2 must be"):
        FR.convert_frames(model, pool, torch.zeros(U + 1, MD))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_convert_frames(hb, dtype):
    pool, win = _mpool()
    _check_convert(_model("fhvae", dtype), pool, win, 64)
    assert hb.lstm_sync_status() == 0


def test_simple_fhvae_frames(hb):
    pool, win = _mpool()
    model = _model("simple")
    _check_encode(model, pool, win, 64)
    _check_convert(model, pool, win, 64)


def test_convert_refuses_a_shift_that_leaves_gaps(hb):
    import frames as FR

    feats, mean, std = _corpus(MF, MLENGTHS, seed=3)
    pool = FR.FramePool(feats, MT, 11, mean, std, device="cuda")
    model = _model("fhvae")
    with pytest.raises(ValueError, match="shift = 11"):
        FR.convert_frames(model, pool)
    z1, _, mu2 = FR.encode_frames(model, pool, batch_size=64)  # latents at any shift
    assert z1.shape[0] == sum(R.n_windows(n, 11) for n in MLENGTHS) and mu2.shape[0] == len(MLENGTHS)
    with pytest.raises(ValueError, match="utterance 1 has no frames"):
        FR.FramePool([feats[0], feats[1][:0]], MT, 1, device="cuda")


# ------------------------------------------------------------------------------------------------------------ the CLI
def test_extract_latents_cli(hb, tmp_path):
    import frames as FR
    import kaldi_io_lite as K
    import utils
    from datasets import KaldiDataset, NumpyDataset
    from fhvae import FHVAE

    keys = ["spk1-a", "one", "spk2-a", "spk2-b"]
    lengths = [45, 1, 19, 130]
    rng = np.random.default_rng(5)
    src = tmp_path / "src"
    src.mkdir()
    with open(src / "feats.scp", "w") as fs, open(src / "len.scp", "w") as ls:
        for k, n in zip(keys, lengths):
            np.save(src / (k + ".npy"), (rng.standard_normal((n, MF)) * 2 + 1).astype(np.float32))
            fs.write("%s %s\n" % (k, src / (k + ".npy")))
            ls.write("%s %d\n" % (k, n))
    torch.manual_seed(5)
    m = FHVAE(MT * MF, [MH, MH], [MH, MH], MD, MD, [MH, MH], seg_len=MT, num_seqs=4)
    utils.save_checkpoint(m, None, [], {}, "t", 1, 1, 0.0, 0.0, str(tmp_path))
    base = [sys.executable, os.path.join(ROOT, "pytorch-scalablefhvae_amd", "extract_latents.py"), "--checkpoint", str(tmp_path / "fhvae_t_e1.tar"),
            "--feat-scp", str(src / "feats.scp"), "--len-scp", str(src / "len.scp"), "--mvn-path", str(tmp_path / "mvn.json"),
            "--what", "z1", "mu2", "convert", "--convert-to", "spk2-a", "--batch-size", "64"]
    outs = {"kaldi": tmp_path / "k", "numpy": tmp_path / "n"}
    for fmt, extra in (("numpy", []), ("kaldi", ["--compress"])):
        r = subprocess.run(base + ["--out", str(outs[fmt]), "--out-format", fmt] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        s = json.load(open(outs[fmt] / "summary.json"))
        assert (s["utterances"], s["frames"], s["windows"], s["shift"], s["T"], s["compute_dtype"]) == (4, sum(lengths), sum(lengths), 1, MT, "f32")
        assert s["written"] == {"z1": 4, "mu2": 4, "convert": 4}
    # what the same calls give in this process
    ds = NumpyDataset(str(src / "feats.scp"), str(src / "len.scp"), 0, str(tmp_path / "mvn.json"), MT, 1, False)
    pool = FR.FramePool(ds, MT, 1, device="cuda")
    model = m.cuda().eval()
    z1, _, mu2 = FR.encode_frames(model, pool, 64)
    conv = FR.convert_frames(model, pool, mu2[2], 64)
    z1_u, conv_u = [a.cpu().numpy() for a in pool.split_windows(z1)], [a.cpu().numpy() for a in pool.split_frames(conv)]
    # numpy: every key, in order, as many z1 rows as the input's len.scp says, bitwise what encode_frames gives
    for what, want in (("z1", z1_u), ("convert", conv_u)):
        got = NumpyDataset(str(outs["numpy"] / what / "feats.scp"), str(outs["numpy"] / what / "len.scp"), 0, None, MT, 1, False)
        assert got.seq_keys == keys and got.seq_lens == lengths
        for i in range(4):
            assert _same(got.load_seq(i), want[i]), (what, i)
    assert open(outs["numpy"] / "mu2" / "keys.txt").read().split() == keys
    assert _same(np.load(outs["numpy"] / "mu2" / "mu2.npy"), mu2.cpu().numpy())
    # kaldi, compressed: the archive decodes to what the host codec makes of those rows; mu2 is a one-row matrix per key
    for what, want in (("z1", z1_u), ("convert", conv_u)):
        got = KaldiDataset(str(outs["kaldi"] / what / "feats.scp"), str(outs["kaldi"] / what / "len.scp"), 0, None, MT, 1, False)
        assert got.seq_keys == keys and got.seq_lens == lengths
        for i in range(4):
            assert K.read_raw(got.seq_feats[i])[0] == ("CM" if lengths[i] > 8 else "CM2")
            tok, payload = K.compress_mat(want[i], "auto")
            assert _same(got.load_seq(i), K.CompressedMatrix(tok, K.header_bytes(want[i]), payload).decode()), (what, i)
    got = KaldiDataset(str(outs["kaldi"] / "mu2" / "feats.scp"), str(outs["kaldi"] / "mu2" / "len.scp"), 0, None, MT, 1, False)
    assert got.seq_keys == keys and got.seq_lens == [1] * 4
    assert _same(np.concatenate([got.load_seq(i) for i in range(4)]), mu2.cpu().numpy())
