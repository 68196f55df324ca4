"""Feature extraction on a MI355X (csrc/feats.hip through features.compute_features and prepare_numpy_data.py): fbank and
spec against the float64 oracle of tests/feats_ref.py at 16, 8 and 22.05 kHz (odd n_fft), bitwise batch invariance, the
status word of inconsistent frame pointers, and the CLI end to end into NumpyDataset, ResidentSegmentPool and training."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import feats_ref as R
from test_feats_cpu import _write_wav, speechlike

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = {"fbank": -20.0, "spec": -50.0}


@pytest.fixture(scope="module")
def F():
    import build_ext

    build_ext.build(verbose=False)
    import features
    import hip_binding

    hip_binding.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return features


def check_against_oracle(got, y, sr, ftype, n_mels=80):
    want = R.features(y, sr, ftype, n_mels=n_mels)
    assert got.dtype == np.float32 and got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want)
    ok = err <= 5e-4
    ok |= np.abs(np.exp(got.astype(np.float64)) - np.exp(want)) <= 1e-6 * np.exp(want).max(axis=1, keepdims=True)
    assert ok.all(), "worst |got - want| = %g at %s" % (err.max(), np.unravel_index(err.argmax(), err.shape))
    # frames whose pre-emphasised, reflected samples are all exactly zero give exactly the floor
    n_fft, hop = R.sizes(sr)
    pre = np.asarray(y, np.float64).copy()
    pre[1:] = y[1:] - 0.97 * np.asarray(y[:-1], np.float64)
    padded = np.pad(pre, n_fft // 2, mode="reflect")
    silent = np.array([not padded[f * hop:f * hop + n_fft].any() for f in range(len(got))])
    assert np.all(got[silent] == FLOOR[ftype])
    return err.max(), int(silent.sum())


@pytest.mark.parametrize("sr", [16000, 8000, 22050])
@pytest.mark.parametrize("ftype", ["fbank", "spec"])
def test_against_oracle(F, sr, ftype):
    n_fft, hop = R.sizes(sr)
    import hip_binding as hb

    tile = hb.load_library().fhvae_feats_tile_rows(n_fft, hb.FEATS_TYPES[ftype])  # frames per workgroup
    assert tile in (16, 32, 64)
    waves = []
    y = speechlike(sr, 1.3, sr)
    y[sr // 4:sr // 4 + 3 * n_fft] = 0.0  # digital silence: several whole frames of exact zeros
    waves.append(y)
    waves.append(speechlike(sr, 0.05, sr + 1)[:n_fft // 2 + 1])  # the shortest utterance accepted
    for nfr in (tile - 1, tile, tile + 1, 2 * tile + 3):  # utterances that put tile boundaries inside them
        L = (nfr - 1) * hop + hop // 2  # exactly nfr frames for even and odd n_fft
        waves.append(speechlike(sr, L / sr + 0.01, sr + nfr)[:L])
    got = F.compute_features(waves, sr, ftype)
    assert len(got) == len(waves)
    worst, silent = 0.0, 0
    for k, (g, w) in enumerate(zip(got, waves)):
        if k >= 2:
            assert len(g) == (tile - 1, tile, tile + 1, 2 * tile + 3)[k - 2]
        assert len(g) == F.num_frames(len(w), n_fft, hop) == R.n_frames(len(w), n_fft, hop)
        e, s = check_against_oracle(g, w, sr, ftype)
        worst, silent = max(worst, e), silent + s
    assert silent >= 2
    print("sr %d %s: worst |got - oracle| %.3g over %d utterances" % (sr, ftype, worst, len(waves)))


def test_batch_invariance_bitwise(F):
    sr = 16000
    rng = np.random.default_rng(7)
    lens = rng.integers(201, 12000, size=200)
    lens[:3] = [201, 202, 360]
    waves = [speechlike(sr, L / sr + 0.01, 1000 + j)[:L] for j, L in enumerate(lens)]
    assert sum(lens) >= 10 ** 6
    for ftype in ("fbank", "spec"):
        together = F.compute_features(waves, sr, ftype)  # one launch (< 2**24 samples)
        alone = F.compute_features(waves, sr, ftype, max_samples=1)  # one launch per utterance
        perm = rng.permutation(len(waves))
        shuffled = F.compute_features([waves[j] for j in perm], sr, ftype)
        for j in range(len(waves)):
            assert np.array_equal(together[j], alone[j]), (ftype, j)
        for k, j in enumerate(perm):
            assert np.array_equal(shuffled[k], together[j]), (ftype, j)


def test_status_word_on_decreasing_frame_ptr(F):
    import hip_binding as hb

    sr, n_fft, hop = 16000, 400, 160
    lens = [3000, 5000, 4000]
    frames = [F.num_frames(L, n_fft, hop) for L in lens]
    wave_ptr = np.concatenate([[0], np.cumsum(lens)])
    good = np.concatenate([[0], np.cumsum(frames)])
    bad = good.copy()
    bad[2] = bad[1] - 5  # decreasing
    dev = torch.device("cuda")
    y = torch.from_numpy(np.concatenate([speechlike(sr, L / sr + 0.01, L)[:L] for L in lens])).to(dev)
    dft = torch.from_numpy(F.dft_basis(n_fft)).to(dev)
    mel = torch.from_numpy(F.mel_basis(sr, n_fft, 80)).to(dev)
    for ptr, want_status in ((bad, hb.FEATS_BAD_PTR), (good, 0)):
        out = torch.full((int(good[-1]), 80), 12345.0, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        hb.feats_fwd(y, torch.from_numpy(wave_ptr).to(dev), torch.from_numpy(ptr).to(dev), dft, mel, n_fft, hop, 80, "fbank", out,
                     status)
        torch.cuda.synchronize()
        assert int(status.item()) == want_status
        o = out.cpu().numpy()
        if want_status:
            assert np.all(o == 12345.0)  # nothing written, in particular not the rows around the bad pointer
        else:
            assert np.all(o < 100) and np.all(o >= -20)


def test_prepare_numpy_data_cli_end_to_end(F, tmp_path, capsys):
    import datasets as D
    import train_model as TM

    sr = 16000
    data = tmp_path / "data"
    rng = np.random.default_rng(3)
    want = {}
    for s, set_name in enumerate(("train", "dev", "test")):
        d = data / set_name
        d.mkdir(parents=True)
        lines = []
        for j in range(5 if set_name == "train" else 2):
            seq = "spk%d_%s_%d" % (j % 2, set_name, j)
            n = int(rng.integers(4000, 16000))
            y = speechlike(sr, n / sr + 0.01, 100 * s + j)[:n]
            q = np.round(y * 32768).astype(np.int64).clip(-32768, 32767)
            if set_name == "train" and j == 1:  # one stereo file: the channel mean is used
                q2 = np.round(0.5 * q).astype(np.int64)
                _write_wav(d / (seq + ".wav"), np.stack([q, q2], axis=1), sr, 2)
                wav = ((q / 32768.0).astype(np.float32) + (q2 / 32768.0).astype(np.float32)) / np.float32(2)
            else:
                _write_wav(d / (seq + ".wav"), q[:, None], sr, 2)
                wav = (q / 32768.0).astype(np.float32)
            want[(set_name, seq)] = wav
            lines.append("%s %s\n" % (seq, d / (seq + ".wav")))
        (d / "wav.scp").write_text("".join(lines))
    out = tmp_path / "np"
    script = os.path.join(ROOT, "pytorch-scalablefhvae_amd", "prepare_numpy_data.py")
    r = subprocess.run([sys.executable, script, str(data), "--np_dir", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for set_name in ("train", "dev", "test"):
        seqs = [k[1] for k in want if k[0] == set_name]
        feats = (out / set_name / "feats.scp").read_text().splitlines()
        lens = (out / set_name / "len.scp").read_text().splitlines()
        assert [l.split()[0] for l in feats] == seqs and [l.split()[0] for l in lens] == seqs
        for fl, ll, seq in zip(feats, lens, seqs):
            path = fl.split(None, 1)[1]
            assert path == os.path.join(str(out / set_name), seq + ".npy")
            x = np.load(path)
            assert x.dtype == np.float32 and x.shape == (int(ll.split()[1]), 80)
            check_against_oracle(x, want[(set_name, seq)], sr, "fbank")
    # the loaders read it
    tr = out / "train"
    ds = D.NumpyDataset(tr / "feats.scp", tr / "len.scp", min_len=20, mvn_path=str(tmp_path / "mvn.json"), seg_len=20, seg_shift=8)
    assert len(ds) == 5 and os.path.exists(tmp_path / "mvn.json")
    pool = D.ResidentSegmentPool(ds)
    assert len(pool) == ds.num_segments and pool.num_seqs == 5
    idxs, x, nsegs = pool.batch(torch.arange(4, device="cuda"))
    assert tuple(x.shape) == (4, 20, 80) and torch.isfinite(x).all()
    # and train_model trains on it
    exp = tmp_path / "exp"
    argv = ["--train-feat-scp", str(tr / "feats.scp"), "--train-len-scp", str(tr / "len.scp"), "--dev-feat-scp",
            str(out / "dev" / "feats.scp"), "--dev-len-scp", str(out / "dev" / "len.scp"), "--mvn-path", str(tmp_path / "mvn.json"),
            "--z1-hus", "16", "16", "--z2-hus", "16", "16", "--x-hus", "16", "16", "--z1-dim", "8", "--z2-dim", "8",
            "--epochs", "1", "--training-batch-size", "8", "--exp-dir", str(exp)]
    rc = TM.main(argv)
    text = capsys.readouterr().out
    assert rc == 0 and "Training complete!" in text, text
    lb = [float(l.split("lower bound:")[1].split()[0]) for l in text.splitlines() if "Validation set lower bound" in l]
    assert len(lb) == 1 and np.isfinite(lb[0])
    assert any(p.name.endswith(".tar") for p in exp.iterdir())
