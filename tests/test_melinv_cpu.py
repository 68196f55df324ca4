"""Mel inversion without a GPU: the float64 oracle (tests/melinv_ref.py) against scipy.optimize.nnls, the band form of the
mel bank and the FISTA constants of features.py against the oracle's, every argument error that is reported before any
launch, the parsers' defaults, and the built library's new entry points."""
import ctypes
import os

import numpy as np
import pytest
import torch

import feats_ref
import melinv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the issue's float64 table at 200 iterations: excess of ||A x - m|| over scipy's optimum relative to ||m|| (worst frame),
# worst |log(A x) - log-mel| over bins above the -20 floor
TABLE_200 = {(16000, 80): (8.7e-7, 4.9e-5), (16000, 40): (2.6e-7, 2.2e-5), (8000, 40): (9.4e-10, 7.3e-7), (22050, 80): (5.6e-6, 3.5e-4)}


@pytest.fixture(scope="module")
def F():
    import features

    assert callable(features.mel_to_spec) and callable(features.synthesize_mel)
    return features


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding as hb

    return hb.load_library()


def problem(sr, n_mels, seconds=1.5, seed=0):
    """-> (log-mel float32-representable (frames, n_mels) float64, M = exp of it, A)"""
    y = R.test_signal(sr, int(seconds * sr), seed)
    lm = feats_ref.features(y, sr, "fbank", n_mels=n_mels).astype(np.float32).astype(np.float64)
    return lm, np.exp(lm), R.bank(sr, n_mels)


@pytest.mark.parametrize("sr,n_mels", R.CONFIGS)
def test_oracle_against_scipy_nnls(F, sr, n_mels):
    """The default step count (features.NNLS_ITERS) reaches the table; the long run reaches scipy's residual."""
    pytest.importorskip("scipy")
    assert F.NNLS_ITERS == 200
    lm, M, A = problem(sr, n_mels)
    assert lm.shape == (151, n_mels) and int((lm <= -20.0).all(axis=1).sum()) >= 3  # (frames of digital silence)
    _, r_opt = R.scipy_optimum(M, A)
    norm = np.linalg.norm(M, axis=1)
    x = R.fista(M, A, F.NNLS_ITERS)
    assert np.all(x >= 0.0) and np.all(np.isfinite(x))
    excess, lerr = float(((R.residual(x, M, A) - r_opt) / norm).max()), R.logmel_error(x, lm, A)
    _, r_long = R.long_run(M, A)
    gap = float((np.abs(r_long - r_opt) / norm).max())
    print("%d / %d: 200 iterations excess %.3g, log-mel error %.3g (table %.3g / %.3g); %d iterations against scipy %.3g"
          % ((sr, n_mels, excess, lerr) + TABLE_200[(sr, n_mels)] + (R.LONG_ITERS, gap)))
    assert excess <= 2.0 * TABLE_200[(sr, n_mels)][0]
    assert lerr <= 2.0 * TABLE_200[(sr, n_mels)][1]
    assert gap <= 1e-6  # licenses the long run as the optimum where scipy is absent


def test_oracle_f32_emulation_and_floor_frames(F):
    """At the default step count the float32 emulation stays close to the float64 run, and an all-floor frame gives a tiny
    x (1.04e-7 at 16 kHz / 80)."""
    lm, M, A = problem(16000, 80)
    x64, k64 = R.fista(M, A, F.NNLS_ITERS, keep=(1, 3, 200))
    x32, k32 = R.fista(M, A, F.NNLS_ITERS, np.float32, keep=(1, 3, 200))
    assert x32.dtype == np.float32 and sorted(k32) == [1, 3, 200] and np.array_equal(k64[200], x64)
    d = R.drift(x32, x64)
    print("float32 emulation drift after 200 iterations: %.3g" % d)
    assert d <= 2e-4  # (7.5e-5 in the issue's run)
    silent = (lm <= -20.0).all(axis=1)
    assert 0.0 < x64[silent].max() <= 1.1e-7
    assert (x64 == 0.0).mean() > 0.002  # exact zeros do occur


@pytest.mark.parametrize("sr", [8000, 16000, 22050, 48000])
@pytest.mark.parametrize("n_mels", [40, 80, 128])
def test_band_of_the_bank_is_exact(F, sr, n_mels):
    n_fft, _ = F.frame_sizes(sr)
    A = F.inversion_bank(sr, n_fft, n_mels)
    assert A.shape == (n_mels, n_fft // 2 + 1) and np.array_equal(A, F.mel_filters(sr, 2 * (n_fft // 2), n_mels))
    band = F.MelBand(A)
    assert np.array_equal(band.dense(), A) and np.array_equal(band.dense_from_bins(), A)
    assert band.filt_off[-1] == len(band.filt_w) == int((A != 0).sum()) <= 2 * band.n_bins
    assert band.bin_filt.dtype == band.filt_first.dtype == band.filt_off.dtype == np.int32
    assert band.bin_filt.min() >= 0 and band.bin_filt.max() < n_mels
    assert np.abs(A - feats_ref.mel_bank(sr, 2 * (n_fft // 2), n_mels)).max() <= 1e-12 * A.max()


def test_a_matrix_that_is_not_banded_is_refused(F):
    A = F.inversion_bank(16000, 400, 80)
    for i, j in ((10, 150), (40, 5)):  # a third filter on a bin / a gap inside a filter's run
        B = A.copy()
        B[i, j] = 0.01
        with pytest.raises(ValueError, match="not banded"):
            F.MelBand(B)
    B = A.copy()
    B[60, int(np.flatnonzero(A[60])[2])] = 0.0  # a hole inside a run
    with pytest.raises(ValueError, match="not banded"):
        F.MelBand(B)
    with pytest.raises(ValueError, match="not banded"):
        F.MelBand(np.ones((4, 9)))
    with pytest.raises(ValueError):
        F.MelBand(np.zeros(7))
    # a filter without bins is legal (too many mels for the rate)
    many = F.MelBand(F.inversion_bank(8000, 200, 128))
    assert (np.diff(many.filt_off) == 0).any()


@pytest.mark.parametrize("sr,n_mels", R.CONFIGS)
def test_constants_against_the_oracle(F, sr, n_mels):
    n_fft, _ = F.frame_sizes(sr)
    A = F.inversion_bank(sr, n_fft, n_mels)
    inv_l, beta = F.nnls_constants(A, 200)
    inv_l_ref, beta_ref = R.constants(R.bank(sr, n_mels), 200)
    assert inv_l.dtype == np.float32 and beta.dtype == np.float32 and beta.shape == (200,)
    assert abs(float(inv_l) - float(inv_l_ref)) <= 2.0 ** -22 * float(inv_l_ref)  # (the two banks differ in the last place)
    assert np.array_equal(beta, beta_ref) and beta[0] == 0.0 and np.all(np.diff(beta) > 0) and beta[-1] < 1.0
    L = np.linalg.eigvalsh(A @ A.T)[-1]
    assert float(inv_l) <= 1.0 / L and float(inv_l) >= (1.0 - 2.0 ** -18) / L


def test_argument_errors_before_launch(F):
    ok = np.zeros((10, 80), np.float32)
    cases = [
        (dict(mels=[np.zeros(80, np.float32)]), "shape"),
        (dict(mels=[ok, np.zeros((1, 80), np.float32)]), "at least 2"),
        (dict(mels=[ok, np.zeros((10, 40), np.float32)]), "n_mels"),
        (dict(mels=[ok], n_mels=40), "n_mels"),
        (dict(mels=[np.zeros((10, 257), np.float32)]), "n_mels"),  # above the kernel's limit
        (dict(mels=[ok], nnls_iters=0), "nnls_iters"),
        (dict(mels=[ok], win_t=0.2), "n_fft"),
        (dict(mels=[ok], hop_t=0.00001), "hop"),
    ]
    for kw, match in cases:
        kw = dict(dict(sr=16000), **kw)
        with pytest.raises(ValueError, match=match):
            F.mel_to_spec(**kw)  # (raised before hip_binding is imported: no GPU is needed to get here)
        with pytest.raises(ValueError, match=match):
            F.synthesize_mel(**kw)
    for kw, match in ((dict(hop_t=0.05), "hop"), (dict(momentum=1.0), "momentum"), (dict(n_iter=-1), "n_iter"),
                      (dict(init_phase=[]), "init_phase"), (dict(init_phase=[np.ones((10, 80), np.complex64)]), "init_phase")):
        with pytest.raises(ValueError, match=match):
            F.synthesize_mel([ok], 16000, **kw)
    assert F.mel_to_spec([], 16000) == [] and F.synthesize_mel([], 16000) == []
    # synthesize itself is unchanged: 80 columns are still refused with the old words
    with pytest.raises(ValueError, match="mel inversion is out of scope"):
        F.synthesize([ok], 16000)


def test_parser_defaults_and_cli_errors(tmp_path, capsys):
    import eval_model
    import invert_numpy_data

    a = invert_numpy_data.build_parser().parse_args(["x.scp", "--out", "o"])
    assert a.ftype == "spec" and a.n_mels == 80 and a.nnls_iters == 200
    e = eval_model.build_parser().parse_args(["--checkpoint", "c", "--out", "o"])
    assert e.wav_ftype == "spec" and e.nnls_iters == 200
    np.save(tmp_path / "a.npy", np.zeros((30, 80), np.float32))
    scp = tmp_path / "feats.scp"
    scp.write_text("a %s\n" % (tmp_path / "a.npy"))
    # without the option: the old refusal; with it, the errors of the inversion come before any launch
    assert invert_numpy_data.main([str(scp), "--out", str(tmp_path / "wav")]) == 1
    assert "mel inversion is out of scope" in capsys.readouterr().err
    assert invert_numpy_data.main([str(scp), "--out", str(tmp_path / "wav"), "--ftype", "fbank", "--nnls_iters", "0"]) == 1
    assert "nnls_iters" in capsys.readouterr().err
    assert invert_numpy_data.main([str(scp), "--out", str(tmp_path / "wav"), "--ftype", "fbank", "--n_mels", "40"]) == 1
    assert "n_mels" in capsys.readouterr().err
    assert eval_model.main(["--checkpoint", "c", "--out", "o", "--feat-scp", str(scp), "--wav-out", str(tmp_path / "w"),
                            "--wav-ftype", "fbank", "--nnls-iters", "0"]) == 1
    assert "nnls-iters" in capsys.readouterr().err


def test_abi_argument_errors_before_launch(lib):
    import hip_binding as hb

    for name in ("fhvae_mel_invert", "fhvae_mel_invert_tile_rows"):
        assert name in hb.SIGNATURES and hasattr(lib, name)
    assert (hb.MELINV_BAD_BAND, hb.MELINV_IN_LOG, hb.MELINV_OUT_LOG) == (1, 1, 2)
    buf = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16  # a host address: never dereferenced here
    NULL, SHAPE, LIMIT = -1, -2, -5
    ok = dict(mel=p, n_frames=7, n_mels=80, n_bins=201, bin_filt=p, bin_w=p, filt_first=p, filt_off=p, filt_w=p, nnz=391, inv_l=0.5,
              beta=p, n_iter=200, flags=3, out=p, status=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.fhvae_mel_invert(a["mel"], a["n_frames"], a["n_mels"], a["n_bins"], a["bin_filt"], a["bin_w"], a["filt_first"],
                                    a["filt_off"], a["filt_w"], a["nnz"], a["inv_l"], a["beta"], a["n_iter"], a["flags"], a["out"],
                                    a["status"], None)

    for name in ("mel", "bin_filt", "bin_w", "filt_first", "filt_off", "filt_w", "beta", "out", "status"):
        assert call(**{name: None}) == NULL, name
    assert call(n_frames=0) == SHAPE and call(n_iter=0) == SHAPE and call(nnz=-1) == SHAPE and call(flags=4) == SHAPE
    assert call(n_mels=0) == LIMIT and call(n_mels=257) == LIMIT and call(n_bins=1) == LIMIT and call(n_bins=1026) == LIMIT
    assert call(nnz=403) == LIMIT and call(inv_l=0.0) == LIMIT and call(inv_l=float("nan")) == LIMIT and call(inv_l=float("inf")) == LIMIT
    assert call(n_iter=1 << 31) == LIMIT
    tr = lib.fhvae_mel_invert_tile_rows
    assert tr(80, 201) == 64 and tr(40, 201) == 64 and tr(40, 101) == 64 and tr(80, 276) == 32 and tr(256, 1025) == 8
    assert tr(0, 201) == 0 and tr(257, 201) == 0 and tr(80, 1) == 0 and tr(80, 1026) == 0
    assert lib.fhvae_abi_version() == 12


def test_binding_refuses_cpu_tensors():
    import hip_binding as hb

    i32 = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hb.mel_invert(torch.zeros(2, 3), i32, torch.zeros(4, 2), i32[:3], i32, torch.zeros(5), 0.5, torch.zeros(2), torch.zeros(2, 4),
                      torch.zeros(1, dtype=torch.int32))
