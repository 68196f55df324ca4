"""Waveform synthesis without a GPU: the float64 oracle's own sanity (tests/synth_ref.py), the padded synthesis basis against
numpy.fft.irfft, the WAV writer, utils.overlap_mean, and every argument error that is reported before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import synth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [(16000, 400, 160), (8000, 200, 80), (22050, 551, 220)]


@pytest.fixture(scope="module")
def F():
    import features

    assert callable(features.synthesize) and callable(features.write_wav)
    return features


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding as hb

    return hb.load_library()


@pytest.mark.parametrize("sr,n_fft,hop", RATES)
def test_oracle_perfect_reconstruction(F, sr, n_fft, hop):
    assert R.sizes(sr) == (n_fft, hop) == F.frame_sizes(sr)
    for frames in (2, 3, 57):
        y = R.speechlike(sr, hop * (frames - 1), 3)
        X = R.stft(y, n_fft, hop, frames)
        assert X.shape == (frames, n_fft // 2 + 1)
        back = R.istft(X, n_fft, hop)
        assert back.shape == y.shape
        err = np.abs(back - y).max()
        print("istft(stft(y)) - y at %d/%d, %d frames: %.3g" % (n_fft, hop, frames, err))
        assert err <= 1e-12
    if n_fft % 2 == 0:  # even n_fft: the oracle's frames are those of the feature oracle without pre-emphasis
        import feats_ref

        y = R.speechlike(sr, hop * 20, 4)
        half = n_fft // 2
        padded = np.pad(y, half, mode="reflect")
        assert feats_ref.n_frames(len(y), n_fft, hop) == 21
        want = np.array([np.fft.rfft(R.window(n_fft) * padded[f * hop:f * hop + n_fft]) for f in range(21)])
        assert np.abs(R.stft(y, n_fft, hop, 21) - want).max() <= 1e-12


def test_oracle_plain_griffin_lim_does_not_diverge():
    """momentum = 0 on the test signal at 400 / 160: the spectral convergence never increases over 40 rounds."""
    sr, n_fft, hop = RATES[0]
    y = R.speechlike(sr, hop * 99, 1)
    S = np.abs(R.stft(y, n_fft, hop, 100))
    trace = []
    R.griffinlim(S, R.unit_phases(0, S.shape), 40, 0.0, n_fft, hop, trace=trace)
    sc = [R.spectral_convergence(w, S, n_fft, hop) for w in trace]
    print("spectral convergence, rounds 0 / 10 / 40: %.4f %.4f %.4f" % (sc[0], sc[10], sc[-1]))
    assert len(sc) == 41
    assert all(b <= a for a, b in zip(sc, sc[1:])), sc
    assert sc[-1] < 0.5 * sc[0]


@pytest.mark.parametrize("n_fft", [400, 200, 551, 16, 17])
def test_synth_basis_is_windowed_irfft(F, n_fft):
    B = F.synth_basis(n_fft)
    n_bins = n_fft // 2 + 1
    KP, K2P = (n_fft + 15) // 16 * 16, (2 * n_bins + 15) // 16 * 16
    assert B.shape == (KP, K2P) and B.dtype == np.float32
    assert not B[n_fft:].any() and not B[:, 2 * n_bins:].any()
    rng = np.random.default_rng(n_fft)
    X = rng.standard_normal((5, n_bins)) + 1j * rng.standard_normal((5, n_bins))
    flat = np.zeros((5, K2P))
    flat[:, 0:2 * n_bins:2], flat[:, 1:2 * n_bins:2] = X.real, X.imag
    got = flat @ B.astype(np.float64).T
    want = np.fft.irfft(X, n=n_fft, axis=1) * R.window(n_fft)
    assert np.abs(got[:, :n_fft] - want).max() <= 1e-6 * np.abs(want).max()
    assert not got[:, n_fft:].any()
    np.testing.assert_allclose(F.window_sq(n_fft), R.window(n_fft) ** 2, rtol=1e-6)
    np.testing.assert_allclose(F.hamming(n_fft), R.window(n_fft), rtol=0, atol=1e-15)


def test_write_wav_round_trip_and_clipping(F, tmp_path):
    rng = np.random.default_rng(0)
    y = rng.uniform(-0.999, 0.999, 4000).astype(np.float32)
    p = tmp_path / "a.wav"
    F.write_wav(p, y, 22050)
    back, sr = F.read_wav(p)
    assert sr == 22050 and back.dtype == np.float32 and back.shape == y.shape
    assert np.abs(back - y).max() <= 1.0 / 32768
    exact = (rng.integers(-32768, 32768, 1000) / 32768.0).astype(np.float32)
    F.write_wav(p, exact, 8000)
    assert np.array_equal(F.read_wav(p)[0], exact)
    F.write_wav(p, np.array([-3.0, -1.0, 0.0, 0.99999, 1.0, 7.5], np.float32), 16000)
    back, _ = F.read_wav(p)
    assert np.array_equal(back, np.array([-1.0, -1.0, 0.0, 32767 / 32768, 32767 / 32768, 32767 / 32768], np.float32))
    with pytest.raises(ValueError, match="non-finite"):
        F.write_wav(p, np.array([0.0, np.nan]), 16000)


@pytest.mark.parametrize("T,shift,nframes", [(20, 8, 100), (20, 8, 61), (20, 20, 80), (5, 1, 9), (20, 7, 20), (20, 8, 27)])
def test_overlap_mean_against_loop(T, shift, nframes):
    import utils

    nseg = (nframes - T) // shift + 1
    rng = np.random.default_rng(T * shift)
    seg = rng.integers(-8, 9, size=(nseg, T, 6)).astype(np.float32)
    got, covered = utils.overlap_mean(torch.from_numpy(seg), T, shift, nframes)
    # the three-line loop, in float32 like the function
    acc, cnt = np.zeros((nframes, 6), np.float32), np.zeros((nframes, 1), np.float32)
    for k in range(nseg):
        acc[k * shift:k * shift + T] += seg[k]
        cnt[k * shift:k * shift + T] += 1
    assert covered == (nseg - 1) * shift + T == int((cnt > 0).sum()) <= nframes
    assert got.dtype == torch.float32 and tuple(got.shape) == (covered, 6)
    assert np.array_equal(got.numpy(), acc[:covered] / cnt[:covered])
    want64, c64 = R.overlap_mean(seg, T, shift, nframes)
    assert c64 == covered and np.abs(got.numpy() - want64).max() <= 1e-6
    with pytest.raises(ValueError):
        utils.overlap_mean(torch.from_numpy(seg), T, T + 1, nframes)
    with pytest.raises(ValueError):
        utils.overlap_mean(torch.from_numpy(seg[:, :-1]), T, shift, nframes)


def test_synthesize_argument_errors_before_launch(F):
    ok = np.zeros((10, 201), np.float32)
    cases = [
        (dict(specs=[np.zeros((10, 200), np.float32)]), "201"),                    # wrong column count for (sr, win_t)
        (dict(specs=[np.zeros((10, 101), np.float32)]), "201"),                    # 8 kHz features at 16 kHz
        (dict(specs=[np.zeros((10, 80), np.float32)]), "mel inversion is out of scope"),  # fbank data
        (dict(specs=[ok, np.zeros((1, 201), np.float32)]), "at least 2"),
        (dict(specs=[np.zeros(201, np.float32)]), "shape"),
        (dict(specs=[ok], win_t=0.2), "n_fft"),                                    # n_fft 3200 > 2048
        (dict(specs=[ok], hop_t=0.00001), "hop"),                                  # hop 0
        (dict(specs=[ok], hop_t=0.05), "hop"),                                     # hop 800 > n_fft 400
        (dict(specs=[ok], momentum=1.0), "momentum"),
        (dict(specs=[ok], preemphasis=1.0), "preemphasis"),
        (dict(specs=[ok], n_iter=-1), "n_iter"),
        (dict(specs=[ok], init_phase=[]), "init_phase"),
        (dict(specs=[ok], init_phase=[np.ones((9, 201), np.complex64)]), "init_phase"),
    ]
    for kw, match in cases:
        kw = dict(dict(sr=16000), **kw)
        with pytest.raises(ValueError, match=match):
            F.synthesize(**kw)  # (raised before hip_binding is imported: no GPU is needed to get here)
    assert F.synthesize([], 16000) == []


def test_synth_abi_argument_errors_before_launch(lib):
    import hip_binding as hb

    for name in ("fhvae_synth_istft", "fhvae_synth_project", "fhvae_synth_deemph", "fhvae_synth_tile_rows"):
        assert name in hb.SIGNATURES and hasattr(lib, name)
    assert hb.SYNTH_BAD_PTR == 1
    buf = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16  # a 16-byte aligned host address: never dereferenced here
    NULL, SHAPE, ALIGN, LIMIT = -1, -2, -4, -5

    ok = dict(spec=p, n_frames=7, wave_ptr=p, frame_ptr=p, U=1, n_samples=960, basis=p, win_sq=p, n_fft=400, hop=160, ws=p,
              out=p, status=p)

    def istft(**kw):
        a = dict(ok, **kw)
        return lib.fhvae_synth_istft(a["spec"], a["n_frames"], a["wave_ptr"], a["frame_ptr"], a["U"], a["n_samples"], a["basis"],
                                     a["win_sq"], a["n_fft"], a["hop"], a["ws"], a["out"], a["status"], None)

    for name in ("spec", "wave_ptr", "frame_ptr", "basis", "win_sq", "ws", "out", "status"):
        assert istft(**{name: None}) == NULL, name
    assert istft(n_fft=2049) == LIMIT and istft(n_fft=1) == LIMIT
    assert istft(hop=0) == SHAPE and istft(hop=-3) == SHAPE and istft(hop=401) == LIMIT
    assert istft(U=0) == SHAPE and istft(n_frames=0) == SHAPE and istft(n_samples=0) == SHAPE
    assert istft(basis=p + 4) == ALIGN and istft(ws=p + 8) == ALIGN

    okp = dict(wave=p, n_samples=960, wave_ptr=p, frame_ptr=p, U=1, n_frames=7, dft=p, mag=p, tprev=p, coef=0.5, n_fft=400,
               hop=160, rebuilt=p, next=p, status=p)

    def project(**kw):
        a = dict(okp, **kw)
        return lib.fhvae_synth_project(a["wave"], a["n_samples"], a["wave_ptr"], a["frame_ptr"], a["U"], a["n_frames"], a["dft"],
                                       a["mag"], a["tprev"], a["coef"], a["n_fft"], a["hop"], a["rebuilt"], a["next"], a["status"],
                                       None)

    for name in ("wave", "wave_ptr", "frame_ptr", "dft", "mag", "next", "status"):
        assert project(**{name: None}) == NULL, name
    assert project(n_fft=2049) == LIMIT and project(n_fft=1) == LIMIT
    assert project(hop=0) == SHAPE and project(hop=401) == LIMIT
    assert project(U=0) == SHAPE and project(n_frames=0) == SHAPE and project(n_samples=0) == SHAPE
    assert project(dft=p + 4) == ALIGN and project(next=p + 4) == ALIGN and project(tprev=p + 4) == ALIGN

    def deemph(wave=p, wave_ptr=p, U=1, n=960, coef=0.97, out=p, status=p):
        return lib.fhvae_synth_deemph(wave, wave_ptr, U, n, coef, out, status, None)

    assert deemph(wave=None) == NULL and deemph(wave_ptr=None) == NULL and deemph(out=None) == NULL and deemph(status=None) == NULL
    assert deemph(U=0) == SHAPE and deemph(n=0) == SHAPE
    assert deemph(coef=1.0) == LIMIT and deemph(coef=-1.5) == LIMIT and deemph(coef=float("nan")) == LIMIT
    assert deemph(coef=0.99999) == LIMIT  # the restart distance for 2^-30 exceeds 65536 samples

    assert lib.fhvae_synth_tile_rows(400) == 64 and lib.fhvae_synth_tile_rows(200) == 64 and lib.fhvae_synth_tile_rows(551) == 64
    assert lib.fhvae_synth_tile_rows(2048) == 16 and lib.fhvae_synth_tile_rows(1) == 0 and lib.fhvae_synth_tile_rows(2049) == 0
    assert lib.fhvae_abi_version() == 12


def test_binding_refuses_cpu_tensors():
    import hip_binding as hb

    z = torch.zeros(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hb.synth_deemph(z, torch.zeros(2, dtype=torch.int64), 0.97, z.clone(), torch.zeros(1, dtype=torch.int32))


def test_eval_and_invert_cli_refuse_bad_input(tmp_path, capsys):
    import invert_numpy_data

    np.save(tmp_path / "a.npy", np.zeros((30, 80), np.float32))
    scp = tmp_path / "feats.scp"
    scp.write_text("a %s\n" % (tmp_path / "a.npy"))
    assert invert_numpy_data.main([str(scp), "--out", str(tmp_path / "wav")]) == 1
    assert "mel inversion is out of scope" in capsys.readouterr().err
    assert invert_numpy_data.main([str(scp), "--out", str(tmp_path / "wav"), "--hop_t", "0.05"]) == 1
    import eval_model

    args = eval_model.build_parser().parse_args(["--checkpoint", "c", "--out", "o"])
    assert args.wav_out is None and args.wav_seqs == 0 and args.gl_iters == 32 and args.sr == 16000
