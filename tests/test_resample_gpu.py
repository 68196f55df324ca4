"""Resampling on a MI355X (csrc/resample.hip through features.resample, compute_features(rates=...) and
prepare_numpy_data.py --resample) against the float64 oracle of tests/resample_ref.py: per-element error in units of
u[t] = 2^-24 * sum_j |h_j| |x_j| (the convention of tests/head_elbo_compare.py), lengths and the zero tail, the status
word of inconsistent pointers, bitwise batch invariance, features of resampled audio, and the CLI end to end.

The statistical bound's yardstick is the reference's own arithmetic: resample_ref.resample_f32_sequential (one product
after the other into a float32 output) on speechlike(sr_in, 0.12, sr_in) reaches, against the oracle, in units of u:
    44100 -> 16000  max 10.18  mean 2.058      8000 -> 16000  max 7.49  mean 1.288
    22050 -> 16000  max  7.02  mean 1.440     16000 -> 22050  max 8.79  mean 1.263
    48000 -> 16000  max 12.65  mean 2.249     11025 -> 16000  max 7.24  mean 1.231
STAT holds twice those values.  The kernel's own figures are printed by test_against_oracle (measured on one MI355X:
max 2.6-3.1, mean 0.43-0.48 for the six pairs); they do not feed back into STAT."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import audio_compare
import feats_ref
import resample_ref as R
from test_resample_cpu import PAIRS, speechlike

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT = {(44100, 16000): (20.36, 4.116), (22050, 16000): (14.04, 2.880), (48000, 16000): (25.30, 4.498),
        (8000, 16000): (14.98, 2.576), (16000, 22050): (17.58, 2.526), (11025, 16000): (14.48, 2.462)}


@pytest.fixture(scope="module")
def F():
    import build_ext

    build_ext.build(verbose=False)
    import features
    import hip_binding

    hip_binding.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return features


def _batch(F, sr_in, sr_out):
    b = F.resample_bank(sr_in, sr_out)
    import hip_binding as hb

    tile = hb.load_library().fhvae_resample_tile_rows(b.KP)
    assert tile in (16, 32, 64)
    row_in = b.P * b.M  # input samples per output row
    waves = [speechlike(sr_in, 0.12, sr_in)]  # (the statistical bound's utterance)
    long = speechlike(sr_in, 1.1, sr_in + 1)
    waves.append(long)  # long: `tile` rows of `row_in` samples per workgroup, so tile boundaries fall inside it or inside the batch
    waves.append(np.array([0.25], np.float32))  # one sample
    for k, d in ((3, 0), (3, 1), (3, -1), (40, 0), (41, 1)):
        waves.append(speechlike(sr_in, (k * b.M + 2) / sr_in + 0.01, sr_in + 10 * k + d)[:k * b.M + d])
    waves.append(np.zeros(2 * b.M + 5, np.float32))  # digital silence
    waves.append(speechlike(sr_in, 0.3, sr_in + 2))
    return b, waves


def _units(got, y, sr_in, sr_out, terms):
    want, cond, taps = R.resample(y, sr_in, sr_out)
    # |got - want| <= (terms + 2) u per element (the comparator all audio kernels share; derivation in its docstring)
    units = audio_compare.dense_units(got, want, 2.0 ** -24 * cond, terms, c=2, what="resample %d -> %d" % (sr_in, sr_out))
    n_calc = R.lengths(len(y), sr_in, sr_out)[0]
    assert not got[n_calc:].any()  # librosa's zero tail past resampy's int(n * ratio)
    return units


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_against_oracle(F, sr_in, sr_out):
    b, waves = _batch(F, sr_in, sr_out)
    got = F.resample(waves, sr_in, sr_out)
    assert len(got) == len(waves)
    worst = 0.0
    for k, (g, y) in enumerate(zip(got, waves)):
        assert len(g) == F.resampled_length(len(y), sr_in, sr_out) == R.lengths(len(y), sr_in, sr_out)[1]
        if len(y) > 30000:
            # the oracle is a Python loop: compare the head of the long utterance through a run of its own on a prefix whose
            # outputs cannot see the cut (the filter's half width is below 64 / min(ratio, 1) input samples)
            cut = 12000
            keep = int(R.lengths(cut, sr_in, sr_out)[0] - (64 / min(b.ratio, 1.0) + 2) * b.ratio)
            want, cond, _ = R.resample(y[:cut], sr_in, sr_out)
            u = 2.0 ** -24 * cond[:keep]
            err = np.abs(g[:keep].astype(np.float64) - want[:keep])
            assert np.all(err <= (b.terms(keep) + 2) * u)
            continue
        e = _units(g, y, sr_in, sr_out, b.terms(len(g)))
        if not np.any(y):
            assert not g.any()  # digital silence: exactly zero
        if len(e):
            worst = max(worst, e.max())
        if k == 0:
            print("%d -> %d: kernel max %.2f mean %.3f units of u (sequential float32 emulation x 2: max %.2f mean %.3f)"
                  % (sr_in, sr_out, e.max(), e.mean(), *STAT[(sr_in, sr_out)]))
            assert e.max() <= STAT[(sr_in, sr_out)][0] and e.mean() <= STAT[(sr_in, sr_out)][1]
    print("%d -> %d: worst element of the batch %.2f units" % (sr_in, sr_out, worst))


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_batch_invariance(F, sr_in, sr_out):
    _, waves = _batch(F, sr_in, sr_out)
    together = F.resample(waves, sr_in, sr_out)
    order = [5, 0, 9, 2, 7, 1, 3, 8, 4, 6]
    assert sorted(order) == list(range(len(waves)))
    shuffled = F.resample([waves[j] for j in order], sr_in, sr_out)
    split = F.resample(waves, sr_in, sr_out, max_samples=1)  # every utterance in a launch of its own
    for k, j in enumerate(order):
        assert np.array_equal(shuffled[k], together[j])
    for a, c in zip(split, together):
        assert np.array_equal(a, c)


def test_bad_pointers_set_status_and_write_nothing(F):
    import hip_binding as hb

    sr_in, sr_out = 44100, 16000
    b = F.resample_bank(sr_in, sr_out)
    lens = np.array([3000, 2000], np.int64)
    olens = F.resampled_length(lens, sr_in, sr_out)
    rows = -(-olens // (b.P * b.L))
    ptr = lambda v: torch.from_numpy(np.concatenate([[0], np.cumsum(v)]).astype(np.int64)).cuda()
    wave = torch.randn(int(lens.sum()), device="cuda")
    bank, chunks = torch.from_numpy(b.bank32).cuda(), torch.from_numpy(b.chunks).cuda()
    exc, alt = torch.from_numpy(b.exceptions(64).copy()).cuda(), torch.from_numpy(b.alt32).cuda()

    def run(in_ptr, out_ptr, row_ptr, n_out):
        out = torch.full((n_out,), 7.0, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        hb.resample_fwd(wave, in_ptr, out_ptr, row_ptr, int(rows.sum()), bank, chunks, b.L, b.M, b.P, b.WL, b.ratio, exc, alt,
                        b.alt_wl, out, status)
        return out.cpu().numpy(), int(status.item())

    n_out = int(olens.sum())
    good, st = run(ptr(lens), ptr(olens), ptr(rows), n_out)
    assert st == 0 and not np.any(good == 7.0)
    want = F.resample([wave[:3000].cpu().numpy(), wave[3000:].cpu().numpy()], sr_in, sr_out)
    assert np.array_equal(good, np.concatenate(want))
    for bad in ("in", "out", "row", "order"):
        i, o, r = lens.copy(), olens.copy(), rows.copy()
        if bad == "in":
            i[0] += 500  # lengths that do not give the outputs' lengths (and run past the input)
        elif bad == "out":
            o[0] -= 1
            o[1] += 1
        elif bad == "row":
            r[0] += 1
            r[1] -= 1
        ip, op, rp = ptr(i), ptr(o), ptr(r)
        if bad == "order":
            ip = ip.flip(0).contiguous()  # not monotone
        out, st = run(ip, op, rp, n_out)
        assert st == hb.RESAMPLE_BAD_PTR, bad
        assert np.all(out == 7.0), bad


def check_against_oracle(got, y, sr, ftype, n_mels=80):
    """(test_feats_gpu.check_against_oracle's tolerance, copied)"""
    want = feats_ref.features(y, sr, ftype, n_mels=n_mels)
    assert got.dtype == np.float32 and got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want)
    ok = err <= 5e-4
    ok |= np.abs(np.exp(got.astype(np.float64)) - np.exp(want)) <= 1e-6 * np.exp(want).max(axis=1, keepdims=True)
    assert ok.all(), "worst |got - want| = %g at %s" % (err.max(), np.unravel_index(err.argmax(), err.shape))
    return err.max()


@pytest.mark.parametrize("ftype", ["fbank", "spec"])
def test_features_of_resampled_audio(F, ftype):
    rates = [44100, 16000, 8000, 22050, 44100, 48000, 11025]
    waves = [speechlike(r, 0.25 + 0.03 * k, r + k) for k, r in enumerate(rates)]
    got = F.compute_features(waves, 16000, ftype, rates=rates)
    assert len(got) == len(waves)
    for k, (g, y, r) in enumerate(zip(got, waves, rates)):
        res = F.resample([y], r, 16000)[0]
        two = F.compute_features([res], 16000, ftype)[0]
        assert np.array_equal(g, two), "utterance %d at %d Hz" % (k, r)  # same kernels; no host round trip in the first
        want, _, _ = R.resample(y, r, 16000)
        check_against_oracle(g, want, 16000, ftype)
    # without rates: today's path, and a waveform already at the target rate takes it either way
    assert np.array_equal(got[1], F.compute_features([waves[1]], 16000, ftype)[0])
    with pytest.raises(ValueError, match="after resampling"):
        F.compute_features([waves[0][:300]], 16000, ftype, rates=[44100], names=["short"])


def test_cli_end_to_end(F, tmp_path):
    from test_feats_cpu import _write_wav

    from datasets import NumpyDataset

    d = tmp_path / "data" / "train"
    d.mkdir(parents=True)
    rates = {"a441": 44100, "b8": 8000, "c16": 16000}
    waves = {}
    for k, (name, sr) in enumerate(rates.items()):
        y = speechlike(sr, 0.4 + 0.1 * k, sr + 5)
        _write_wav(d / (name + ".wav"), np.round(y.astype(np.float64) * 32768).astype(np.int64).reshape(-1, 1), sr, 2)
        waves[name] = y
    (d / "wav.scp").write_text("".join("%s %s\n" % (n, d / (n + ".wav")) for n in rates))
    script = os.path.join(ROOT, "pytorch-scalablefhvae_amd", "prepare_numpy_data.py")
    out = tmp_path / "np"
    r = subprocess.run([sys.executable, script, str(tmp_path / "data"), "--np_dir", str(out), "--set_name", "train", "--resample",
                        "--sr", "16000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    n_fft, hop = F.frame_sizes(16000)
    lens = dict(line.split() for line in (out / "train" / "len.scp").read_text().splitlines())
    for name, sr in rates.items():
        feat = np.load(out / "train" / (name + ".npy"))
        y, sr_file = F.read_wav(d / (name + ".wav"))
        assert sr_file == sr
        want, _, _ = R.resample(y, sr, 16000)
        assert feat.shape == (F.num_frames(len(want), n_fft, hop), 80) and int(lens[name]) == len(feat)
        check_against_oracle(feat, want, 16000, "fbank")
    ds = NumpyDataset(str(out / "train" / "feats.scp"), str(out / "train" / "len.scp"))
    assert sorted(ds.seqlist) == sorted(rates) and [ds.lens[n] for n in rates] == [int(lens[n]) for n in rates]
    # the 16 kHz file alone, without the flag: the same bytes
    d2 = tmp_path / "data2" / "train"
    d2.mkdir(parents=True)
    (d2 / "wav.scp").write_text("c16 %s\n" % (d / "c16.wav"))
    r = subprocess.run([sys.executable, script, str(tmp_path / "data2"), "--set_name", "train"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    assert (d2 / "c16.npy").read_bytes() == (out / "train" / "c16.npy").read_bytes()
    # without --resample the mixed corpus is still refused
    r = subprocess.run([sys.executable, script, str(tmp_path / "data"), "--np_dir", str(tmp_path / "np2"), "--set_name", "train",
                        "--sr", "16000"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "sample rate" in r.stderr
