"""Kaldi filterbank features on a MI355X (csrc/kaldi_fbank.hip through features.compute_kaldi_fbank and
prepare_kaldi_data.py) against the float64 oracle of tests/kaldi_fbank_ref.py.

The bound of every parity check is 4 x the worst error of the oracle's float32 model of the same steps against the float64
oracle on the same input (+ 1e-6), computed here at run time; it is never taken from the kernel's output.  Measured on the
MI355X: see DESIGN section 14."""
import glob
import os
import zlib

import numpy as np
import pytest
import torch

import kaldi_fbank_ref as R
from test_feats_cpu import _write_wav

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "tests", "golden", "kaldi_fbank.conf")
FLOOR32 = np.float32(np.log(2.0 ** -23))


@pytest.fixture(scope="module")
def F():
    import build_ext

    build_ext.build(verbose=False)
    import features
    import hip_binding

    hip_binding.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return features


def opts_of(kw):
    """Oracle keyword arguments -> the option dict of features.kaldi_fbank_options."""
    names = {"sr": "sample-frequency", "window": "window-type", "n_mels": "num-mel-bins", "use_log": "use-log-fbank",
             "use_power": "use-power", "dither": "dither", "low": "low-freq", "high": "high-freq", "remove_dc": "remove-dc-offset",
             "preemph": "preemphasis-coefficient"}
    o = {"dither": 0.0}
    o.update({names[k]: v for k, v in kw.items()})
    return o


def compare(got, want, model, use_log=True, what=""):
    """Every element of got (kernel) against want (float64 oracle) within 4 x the float32 model's worst error + 1e-6."""
    assert got.dtype == np.float32 and got.shape == want.shape == model.shape
    if use_log:
        scale = 1.0
    else:  # linear energies: relative to the frame's largest energy
        scale = np.maximum(want.max(axis=1, keepdims=True), 1.0)  # (silent frames: energy 0)
    bound = 4.0 * (np.abs(model.astype(np.float64) - want) / scale).max() + 1e-6
    err = np.abs(got.astype(np.float64) - want) / scale
    print("%s: worst kernel error %.3g, float32 model %.3g, bound %.3g" % (what, err.max(), (bound - 1e-6) / 4, bound))
    assert err.max() <= bound, "%s: worst |got - want| = %g at %s, bound %g" % (what, err.max(), np.unravel_index(err.argmax(), err.shape), bound)
    return err.max()


CASES = [dict(window="hamming", n_mels=80), dict(window="povey", n_mels=23), dict(window="hanning", n_mels=40),
         dict(window="rectangular", n_mels=80), dict(window="blackman", n_mels=40), dict(window="hamming", n_mels=40, sr=8000),
         dict(window="povey", n_mels=23, sr=8000), dict(window="hamming", n_mels=80, use_power=False),
         dict(window="hamming", n_mels=80, use_log=False), dict(window="povey", n_mels=40, low=100.0, high=-400.0, preemph=0.0),
         dict(window="hamming", n_mels=80, remove_dc=False)]


@pytest.mark.parametrize("kw", CASES, ids=lambda kw: "-".join("%s=%s" % kv for kv in kw.items()))
def test_parity_without_dither(F, kw):
    sr = kw.get("sr", 16000)
    y = R.probe(sr)
    want = R.fbank(y, **kw)
    model = R.fbank_f32(y, **kw)
    got = F.compute_kaldi_fbank([(y / 32768.0).astype(np.float32)], opts_of(kw))[0]
    N, S, P = R.sizes(sr)
    assert len(got) == R.n_frames(len(y), N, S) == 198
    compare(got, want, model, kw.get("use_log", True), str(kw))
    if kw.get("use_log", True) and kw.get("remove_dc", True):
        floor = want == np.log(R.FLT_EPSILON)
        assert floor.all(axis=1).sum() >= 80  # digital silence and the constant offset
        assert np.all(got[floor] == FLOOR32) and np.array_equal(got == FLOOR32, floor)
        # dither = 0 does not touch the generator: any seed and stream id give the same bits
        again = F.compute_kaldi_fbank([(y / 32768.0).astype(np.float32)], opts_of(kw), seed=99, stream_ids=[7])[0]
        assert np.array_equal(got, again)


def test_parity_with_dither(F):
    kw = dict(window="hamming", n_mels=80, dither=1.0)
    y = R.probe()
    N, S, P = R.sizes(16000)
    seed, sid = 0x1234567890ABCDEF, 0xFEDCBA9876543210
    g = R.noise(seed, sid, R.n_frames(len(y), N, S), N)
    want = R.fbank(y, noise_in=g, **kw)
    assert np.array_equal(want, R.fbank(y, seed=seed, stream_id=sid, **kw))
    model = R.fbank_f32(y, noise_in=g.astype(np.float32), **kw)  # f32 Box-Muller is within a rounding of this noise
    yw = (y / 32768.0).astype(np.float32)
    got = F.compute_kaldi_fbank([yw], opts_of(kw), seed=seed, stream_ids=[sid])[0]
    compare(got, want, model, True, "dither 1")
    assert not np.any(got == FLOOR32)
    # the same (seed, stream id) gives the same bits; another seed or another stream id does not
    assert np.array_equal(got, F.compute_kaldi_fbank([yw], opts_of(kw), seed=seed, stream_ids=[sid])[0])
    other_seed = F.compute_kaldi_fbank([yw], opts_of(kw), seed=seed + 1, stream_ids=[sid])[0]
    other_id = F.compute_kaldi_fbank([yw], opts_of(kw), seed=seed, stream_ids=[sid + (1 << 40)])[0]
    silent = np.all(R.fbank(y, window="hamming", n_mels=80) == np.log(R.FLT_EPSILON), axis=1)
    for o in (other_seed, other_id):
        assert (o[silent] != got[silent]).mean() > 0.99
    # default stream ids are the positions in the list
    two = F.compute_kaldi_fbank([yw, yw], opts_of(kw), seed=seed)
    assert not np.array_equal(two[0], two[1])
    assert np.array_equal(two[1], F.compute_kaldi_fbank([yw], opts_of(kw), seed=seed, stream_ids=[1])[0])


SILENT_FRAMES = 2000
SEEDS_KERNEL, SEEDS_ORACLE = (11, 12, 13, 14), (21, 22, 23, 24)  # 500 frames each; constants, so the test is deterministic


def _oracle_silent(seeds):
    """Per-frame mean log-energy of silent input under dither 1, 500 frames per seed."""
    N, S, P = R.sizes(16000)
    n = N + (SILENT_FRAMES // len(seeds) - 1) * S
    return np.concatenate([R.fbank(np.zeros(n), seed=s, stream_id=5, window="hamming", n_mels=80, dither=1.0).mean(axis=1) for s in seeds])


def test_dither_statistics_on_silence(F):
    """All-zero input: the features are those of N(0, 1) samples.  The mean log-energy of 2000 frames from the kernel lies
    within 3 standard errors of the oracle's over an independent seed set (the oracle against itself on the two sets: passes)."""
    N, S, P = R.sizes(16000)
    n = N + (SILENT_FRAMES // len(SEEDS_KERNEL) - 1) * S
    o = opts_of(dict(window="hamming", n_mels=80, dither=1.0))
    a = np.concatenate([F.compute_kaldi_fbank([np.zeros(n, np.float32)], o, seed=s, stream_ids=[5])[0].astype(np.float64).mean(axis=1)
                        for s in SEEDS_KERNEL])
    b = _oracle_silent(SEEDS_ORACLE)
    assert len(a) == len(b) == SILENT_FRAMES
    se = np.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
    print("silence: kernel mean %.5f, oracle mean %.5f, standard error %.5f" % (a.mean(), b.mean(), se))
    assert abs(a.mean() - b.mean()) <= 3 * se


def test_batch_independence_bitwise(F):
    rng = np.random.default_rng(7)
    N, S, P = R.sizes(16000)
    tile = __import__("hip_binding").load_library().fhvae_kaldi_fbank_tile_rows(N, P, 80)
    assert tile in (16, 32, 48, 64)
    lens = rng.integers(N, 12000, size=200)
    lens[:6] = [N, N + 1, N + S - 1, N + S, N + (tile - 1) * S, N + tile * S]  # one frame; tiles ending at utterance ends
    waves = [(R.probe(16000, L / 16000 + 0.01, 1000 + j)[:L] / 32768.0).astype(np.float32) for j, L in enumerate(lens)]
    ids = [zlib.crc32(b"utt%d" % j) for j in range(len(waves))]
    for dither in (0.0, 1.0):
        o = opts_of(dict(window="hamming", n_mels=80, dither=dither))
        together = F.compute_kaldi_fbank(waves, o, seed=3, stream_ids=ids)  # one launch
        alone = F.compute_kaldi_fbank(waves, o, seed=3, stream_ids=ids, max_samples=1)  # one launch per utterance
        perm = rng.permutation(len(waves))
        shuffled = F.compute_kaldi_fbank([waves[j] for j in perm], o, seed=3, stream_ids=[ids[j] for j in perm])
        assert together[0].shape == (1, 80)
        for j in range(len(waves)):
            assert len(together[j]) == R.n_frames(lens[j], N, S)
            assert np.array_equal(together[j], alone[j]), (dither, j)
        for k, j in enumerate(perm):
            assert np.array_equal(shuffled[k], together[j]), (dither, j)
    # the one-frame utterance against the oracle
    want = R.fbank(waves[0].astype(np.float64) * 32768, window="hamming", n_mels=80)
    model = R.fbank_f32(waves[0] * np.float32(32768), window="hamming", n_mels=80)
    compare(F.compute_kaldi_fbank(waves[:1], opts_of(dict(window="hamming", n_mels=80)))[0], want, model, True, "one frame")


def test_status_word_on_bad_pointers(F):
    import hip_binding as hb

    N, S, P = 400, 160, 512
    lens = [3000, 5000, 4000]
    frames = [R.n_frames(L, N, S) for L in lens]
    wave_ptr = np.concatenate([[0], np.cumsum(lens)])
    good = np.concatenate([[0], np.cumsum(frames)])
    dec = good.copy()
    dec[2] = dec[1] - 5  # decreasing
    more = good.copy()
    more[1:] += 1  # one frame more than the first utterance holds
    dev = torch.device("cuda")
    y = torch.from_numpy(np.concatenate([R.probe(16000, L / 16000 + 0.01, L)[:L] for L in lens]).astype(np.float32)).to(dev)
    dft = torch.from_numpy(F.kaldi_dft_basis(N, P, "hamming")).to(dev)
    mel = torch.from_numpy(F.kaldi_mel_basis(16000, P, 80)).to(dev)
    for ptr, want_status in ((dec, hb.KALDI_BAD_PTR), (more, hb.KALDI_BAD_PTR), (good, 0)):
        out = torch.full((int(ptr[-1]), 80), 12345.0, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        hb.kaldi_fbank_fwd(y, torch.from_numpy(wave_ptr).to(dev), torch.from_numpy(ptr).to(dev), None, dft, mel, N, S, P, 80, 0.97, 0.0, 0,
                           7, out, status)
        torch.cuda.synchronize()
        assert int(status.item()) == want_status
        o = out.cpu().numpy()
        if want_status:
            assert np.all(o == 12345.0)  # nothing written
        else:
            assert np.all(o < 100) and np.all(o >= FLOOR32)


def test_short_utterance_is_named(F):
    with pytest.raises(ValueError, match="tiny.wav.*399 samples"):
        F.compute_kaldi_fbank([np.zeros(8000, np.float32), np.zeros(399, np.float32)], CONF, names=["a.wav", "tiny.wav"])


def test_prepare_kaldi_data_end_to_end(F, tmp_path, capsys):
    import datasets as D
    import eval_model as EM
    import kaldi_io_lite as K
    import prepare_kaldi_data as PK
    import train_model as TM

    sr = 16000
    data = tmp_path / "data"
    rng = np.random.default_rng(3)
    waves = {}
    for s, set_name in enumerate(("train", "dev")):
        d = data / set_name
        d.mkdir(parents=True)
        lines = []
        for j in range(5 if set_name == "train" else 2):
            key = "spk%d_%s_%d" % (j % 2, set_name, j)
            n = int(rng.integers(6000, 16000))
            q = R.probe(sr, n / sr + 0.01, 100 * s + j)[:n].astype(np.int64)
            if set_name == "train" and j == 1:  # a stereo file: channel 0 is used
                _write_wav(d / (key + ".wav"), np.stack([q, q // 2], axis=1), sr, 2)
            else:
                _write_wav(d / (key + ".wav"), q[:, None], sr, 2)
            waves[(set_name, key)] = (q / 32768.0).astype(np.float32)
            lines.append("%s %s\n" % (key, d / (key + ".wav")))
        (d / "wav.scp").write_text("".join(lines))
    for set_name in ("train", "dev"):
        assert PK.main([str(data), "--fbank_conf", CONF, "--set_name", set_name, "--seed", "17", "--kaldi_root", "/nowhere"]) == 0
    assert "--kaldi_root is ignored" in capsys.readouterr().out
    o = F.kaldi_fbank_options(CONF)
    for set_name in ("train", "dev"):
        keys = [k[1] for k in waves if k[0] == set_name]
        want = F.compute_kaldi_fbank([waves[(set_name, k)] for k in keys], o, seed=17, stream_ids=[zlib.crc32(k.encode()) for k in keys])
        scp = (data / set_name / "feats.scp").read_text().splitlines()
        lens = (data / set_name / "len.scp").read_text().splitlines()
        assert [l.split()[0] for l in scp] == keys
        assert lens == ["%s %d" % (k, len(w)) for k, w in zip(keys, want)]
        for line, w in zip(scp, want):
            m = K.load_mat(line.split(None, 1)[1])
            assert m.dtype == np.float32 and m.shape[1] == 80 and np.array_equal(m, w)
        assert [k for k, _ in K.read_ark(data / set_name / "feats.ark")] == keys
    # the same matrices as .npy files: the format does not change a number
    tr = data / "train"
    with open(tmp_path / "np.scp", "w") as fh:
        for key, m in K.read_ark(tr / "feats.ark"):
            np.save(tmp_path / (key + ".npy"), m)
            fh.write("%s %s\n" % (key, tmp_path / (key + ".npy")))
    kd = D.KaldiDataset(tr / "feats.scp", tr / "len.scp", min_len=20, mvn_path=str(tmp_path / "mvn.json"), seg_len=20, seg_shift=8)
    nd = D.NumpyDataset(tmp_path / "np.scp", tr / "len.scp", min_len=20, mvn_path=str(tmp_path / "mvn_np.json"), seg_len=20, seg_shift=8)
    kp, npool = D.ResidentSegmentPool(kd), D.ResidentSegmentPool(nd)
    assert len(kp) == len(npool) == kd.num_segments and torch.equal(kp.pool, npool.pool)
    first = torch.arange(8, device="cuda")
    for a, b in zip(kp.batch(first), npool.batch(first)):
        assert torch.equal(a, b)
    # train_model and eval_model read the archives
    exp = tmp_path / "exp"
    argv = ["--data-format", "kaldi", "--train-feat-scp", str(tr / "feats.scp"), "--train-len-scp", str(tr / "len.scp"),
            "--dev-feat-scp", str(data / "dev" / "feats.scp"), "--dev-len-scp", str(data / "dev" / "len.scp"),
            "--mvn-path", str(tmp_path / "mvn.json"), "--z1-hus", "16", "16", "--z2-hus", "16", "16", "--x-hus", "16", "16",
            "--z1-dim", "8", "--z2-dim", "8", "--epochs", "1", "--training-batch-size", "8", "--exp-dir", str(exp)]
    rc = TM.main(argv)
    text = capsys.readouterr().out
    assert rc == 0 and "Training complete!" in text and "KaldiDataset: 5 out of 5 kept" in text, text
    lb = [float(l.split("lower bound:")[1].split()[0]) for l in text.splitlines() if "Validation set lower bound" in l]
    assert len(lb) == 1 and np.isfinite(lb[0])
    cks = sorted(glob.glob(str(exp / "*.tar")))
    assert cks
    ev = tmp_path / "ev"
    rc = EM.main(["--checkpoint", cks[0], "--out", str(ev), "--data-format", "kaldi", "--feat-scp", str(tr / "feats.scp"),
                  "--len-scp", str(tr / "len.scp"), "--mvn-path", str(tmp_path / "mvn.json"), "--max-recon", "2"])
    assert rc == 0 and os.path.exists(ev / "summary.json")
