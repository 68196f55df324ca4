"""Float64 numpy oracle of the mel inversion (mel magnitudes -> linear magnitudes), independent of features.py: the bank
comes from tests/feats_ref.mel_bank.

Per frame:  minimise ||A x - m||^2 over x >= 0,  A (n_mels, n_bins) the slaney bank the "fbank" features were taken with,
m = exp(log-mel frame).  The minimiser is not unique (A is wide, and rank deficient at 16 kHz / 80 mels), A x and the residual
are.  The algorithm is therefore fixed: FISTA from zero,

    x = y = 0, t = 1;   g = A^T (A y - m);   x+ = max(y - g / L, 0);   t+ = (1 + sqrt(1 + 4 t^2)) / 2;
    y = x+ + ((t - 1) / t+) (x+ - x)

with L = lambda_max(A A^T) (eigvalsh, float64), nudged up by one part in 2**20 before 1 / L is rounded to float32, and the
momentum factors tabulated in float64 and rounded to float32: `constants`.  Every run below uses those float32 constants, so
that the float64 run and the float32 emulation differ in the arithmetic alone.

  fista(M, A, n_iter, dtype, keep)   the iteration on all frames at once; dtype float32 rounds every array and every product
                                     to float32 (the emulation the GPU tests take their drift floor from); `keep`: iteration
                                     counts whose x is returned as well
  optimum(M, A)                      per frame (x, residual norm) of the exact solver scipy.optimize.nnls where scipy is
                                     importable, else of a long float64 run (LONG_ITERS iterations), which the CPU test pins
                                     to scipy's residual within 1e-6 ||m||
"""
import numpy as np

import feats_ref

LONG_ITERS = 5000
CONFIGS = [(16000, 80), (16000, 40), (8000, 40), (22050, 80)]  # sr, n_mels


def bank(sr, n_mels, win_t=0.025):
    n_fft = int(sr * win_t)
    return feats_ref.mel_bank(sr, 2 * (n_fft // 2), n_mels)


def constants(A, n_iter):
    """-> (inv_l, beta (n_iter,)) as float32."""
    L = float(np.linalg.eigvalsh(A @ A.T)[-1])
    inv_l = np.float32(1.0 / (L * (1.0 + 2.0 ** -20)))
    assert float(inv_l) <= 1.0 / L
    beta, t = [], 1.0
    for _ in range(n_iter):
        tn = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        beta.append((t - 1.0) / tn)
        t = tn
    return inv_l, np.asarray(beta, dtype=np.float64).astype(np.float32)


def fista(M, A, n_iter, dtype=np.float64, keep=()):
    """M (frames, n_mels) mel magnitudes -> x (frames, n_bins) after n_iter iterations, in `dtype`; with `keep` a dict
    {iterations: x} as well (n_iter included)."""
    inv_l, beta = constants(A, n_iter)
    A = np.asarray(A, dtype=np.float64).astype(dtype)
    M = np.asarray(M, dtype=np.float64).astype(dtype)
    step = dtype(inv_l)
    x = np.zeros((M.shape[0], A.shape[1]), dtype=dtype)
    y = x.copy()
    kept = {}
    for k in range(n_iter):
        g = ((y @ A.T - M) @ A).astype(dtype)
        xn = np.maximum(y - step * g, dtype(0.0)).astype(dtype)
        y = (xn + dtype(beta[k]) * (xn - x)).astype(dtype)
        x = xn
        if k + 1 in keep:
            kept[k + 1] = x.copy()
    assert x.dtype == dtype and y.dtype == dtype
    return (x, kept) if keep else x


def have_scipy():
    try:
        import scipy.optimize  # noqa: F401
    except ImportError:
        return False
    return True


def scipy_optimum(M, A):
    """Per frame the exact non-negative least squares: (x (frames, n_bins), residual norms (frames,))."""
    from scipy.optimize import nnls

    xs, rs = [], []
    for m in np.asarray(M, dtype=np.float64):
        x, r = nnls(A, m, maxiter=30 * A.shape[1])
        xs.append(x), rs.append(r)
    return np.asarray(xs), np.asarray(rs)


def long_run(M, A):
    x = fista(M, A, LONG_ITERS)
    return x, residual(x, M, A)


def optimum(M, A):
    return scipy_optimum(M, A) if have_scipy() else long_run(M, A)


def residual(x, M, A):
    """||A x - m|| per frame, in float64."""
    return np.linalg.norm(np.asarray(x, np.float64) @ A.T - np.asarray(M, np.float64), axis=1)


def logmel_error(x, logmel, A, floor=-20.0):
    """Worst |log(A x) - log-mel| over the bins whose log-mel lies above the floor (float64)."""
    logmel = np.asarray(logmel, dtype=np.float64)
    with np.errstate(divide="ignore"):
        got = np.log(np.asarray(x, np.float64) @ A.T)
    sel = logmel > floor
    return float(np.abs(got - logmel)[sel].max()) if sel.any() else 0.0


def drift(x, ref):
    """max |x - ref| over the frame's largest reference magnitude, worst frame."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(x - ref).max(axis=1) / ref.max(axis=1)).max())


def test_signal(sr, n, seed):
    """Speech-like int16 samples (as float in [-1, 1)) with a stretch of digital silence in the middle: frames that lie
    wholly inside it are all-floor."""
    from synth_ref import speechlike

    y = np.round(speechlike(sr, n, seed) * 32768.0).clip(-32768, 32767) / 32768.0
    if n >= 8 * int(sr * 0.025):
        a = n // 2
        y[a:a + min(n // 4, int(0.095 * sr))] = 0.0
    return y
