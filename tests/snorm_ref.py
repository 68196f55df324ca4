"""float64 numpy oracle of score normalisation (csrc/snorm.hip, csrc/spk.hip's NormScore, score_norm.py); it shares no code with
score_norm.py.  The cohort statistics come from a full sort of every row and the textbook formulas (the mean and the population
standard deviation of the K largest scores).

THE BOUNDS (derived, not tuned).  U = 2^-24.

  The cohort score s(i, n) = v_i . z_n + a_i + az_n + c in f32 is within
      e(i, n) = U (Dp + 3) (sum_k |v_ik z_nk| + |a_i| + |az_n| + |c|)
  of the float64 one (Dp fma roundings of the dot, the additions: tests/spk_ref.py's delta without the bin terms);
  eps_i = max_n e(i, n).  Sorting is 1-Lipschitz in the sup norm: if every |s'_n - s_n| <= eps, the k-th largest of s' is within
  eps of the k-th largest of s (at least k of the s' lie at or above (k-th largest of s) - eps, and at least Nc - k + 1 at or
  below it + eps).  So the sorted top-K vectors t', t obey |t'_k - t_k| <= eps for every k, and
      |thr' - thr| <= eps                                  (thr is the K-th entry; the device rounds nothing more)
      |mean(t') - mean(t)| <= eps                          (an average of the entries)
      |sd(t') - sd(t)| <= eps                              (sd(t) = |t - mean(t) 1| / sqrt(K); the centring I - 11^T / K is an
                                                            orthogonal projection, so by the triangle inequality the difference
                                                            is at most |t' - t| / sqrt(K) <= eps)
  The device computes mean and variance of the exact f32 scores in float64 (errors of order 2^-53 K, nothing beside U), then
  rounds mu and sd once to f32: 2^-24 |mu| and 2^-24 sd more.  r = 1 / sd is a correctly rounded f32 division: the test holds it
  to float32(1) / sd bit for bit.

  The normalised score on the device's own f32 mu, r (they are inputs of that kernel, exact in float64):
      sn = 0.5 ((s - mu_i) r_i + (s - mu_j) r_j)
  The f32 s is within delta_ij = U (Dp + 3) M_ij of the float64 one (tests/spk_ref.py), which moves sn by at most
  1/2 (r_i + r_j) delta_ij.  Each half then takes one rounding of the subtraction and one of the product, the sum one more (the
  halving is exact): to first order each half's magnitude |s - mu| r times 3 U, halved: 3/2 U (|s - mu_i| r_i + |s - mu_j| r_j).
  The bin arithmetic adds spk_ref's four roundings, 4 U (hi - lo):
      Delta_ij = 1/2 (r_i + r_j) delta_ij + 3/2 U (|s - mu_i| r_i + |s - mu_j| r_j) + 4 U (hi - lo)
"""
import numpy as np

import spk_ref as R

U = R.U


# ------------------------------------------------------------------------------------------------------- cohort statistics
def cohort_scores(v, a, z, az, c):
    """-> (s (S, Nc) float64, eps (S,)): the cohort scores on the f32 operands and the per-row bound on the f32 score's error."""
    v, a, z, az = (np.asarray(t, dtype=np.float64) for t in (v, a, z, az))
    s = v @ z.T + a[:, None] + az[None, :] + float(c)
    M = np.abs(v) @ np.abs(z).T + np.abs(a)[:, None] + np.abs(az)[None, :] + abs(float(c))
    return s, U * (v.shape[1] + 3) * M.max(axis=1)


def top_k(top, Nc):
    return Nc if top <= 0 else min(int(top), Nc)


def stats(s, top):
    """s (S, Nc) float64 -> (thr, mu, sd) (S,) float64 of each row's K = top_k(top, Nc) largest: a full sort per row, the mean
    and the population standard deviation by the textbook."""
    s = np.asarray(s, dtype=np.float64)
    K = top_k(top, s.shape[1])
    t = -np.sort(-s, axis=1)[:, :K]
    mu = t.sum(axis=1) / K
    sd = np.sqrt(((t - mu[:, None]) ** 2).sum(axis=1) / K)
    return t[:, K - 1].copy(), mu, sd


def stats_bounds(eps, mu, sd):
    """-> the allowances of (thr, mu, sd) for the bound eps (S,) on the scores' errors."""
    return eps, eps + U * np.abs(mu), eps + U * sd


# -------------------------------------------------------------------------------------------------------- normalised score
def normalise(s, mu, r, i, j):
    """float64 sn of the trials (i, j) with scores s, from the (S,) statistics mu and r = 1 / sd."""
    mu, r = np.asarray(mu, dtype=np.float64), np.asarray(r, dtype=np.float64)
    return 0.5 * ((s - mu[i]) * r[i] + (s - mu[j]) * r[j])


def norm_delta(s, M, Dp, mu, r, i, j, lo=0.0, hi=0.0):
    """Delta_ij of the module docstring, per trial."""
    mu, r = np.asarray(mu, dtype=np.float64), np.asarray(r, dtype=np.float64)
    return (0.5 * (r[i] + r[j]) * R.delta(M, Dp) + 1.5 * U * (np.abs(s - mu[i]) * r[i] + np.abs(s - mu[j]) * r[j])
            + 4.0 * U * (float(hi) - float(lo)))


# ------------------------------------------------------------------------------------------------------------------ the data
def two_conditions(seed=7, shift_norm=4.0):
    """The set the end-to-end tests rest on: a PLDA fitted on ONE condition (planted(132, 120, 20, 32, nuisance=0), length
    normalisation, 5 iterations), 30 held-out speakers of 25 rows of which every second row is shifted by one fixed direction of
    norm `shift_norm`, and a cohort of 600 unlabelled rows of 60 other speakers (10 each), every second one shifted the same way
    -> dict: model (the oracle's fit), x, label (evaluation), cohort (600, 32)."""
    K = 32
    xt, lt = R.planted(132, 120, 20, K, nuisance=0)
    model = R.fit(xt, lt, None, True, iters=5)
    direction = np.random.RandomState(seed).randn(K)
    direction *= shift_norm / np.linalg.norm(direction)
    x, label = R.planted(seed + 1, 30, 25, K, nuisance=0, spread=0)
    zc, _ = R.planted(seed + 2, 60, 10, K, nuisance=0, spread=0)
    x, zc = x.astype(np.float64), zc.astype(np.float64)
    x[::2] += direction
    zc[::2] += direction
    return {"model": model, "x": x.astype(np.float32), "label": label, "cohort": zc.astype(np.float32)}


def unit_rows(x):
    """(N, D) -> f32 rows of unit length, zero-padded to a multiple of 16, and a = 0 (what the cosine back ends score)."""
    x = np.asarray(x, dtype=np.float64)
    x = x / np.maximum(np.sqrt((x * x).sum(axis=1)), 1e-30)[:, None]
    out = np.zeros((x.shape[0], (x.shape[1] + 15) // 16 * 16), dtype=np.float32)
    out[:, :x.shape[1]] = x
    return out, np.zeros(x.shape[0], dtype=np.float32)
