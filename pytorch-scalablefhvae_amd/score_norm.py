"""score_norm.py -- score normalisation against a cohort for the speaker back end (include/fhvae_snorm.h): S-norm
with the whole cohort, adaptive S-norm (AS-norm) with the top K cohort scores of either side.

  cohort_stats     per evaluation row the mean and standard deviation of its K largest cohort scores, in one launch with no
                   (S, Nc) matrix (csrc/snorm.hip) -> (mu, sd, r = 1 / sd, thr = the K-th largest score)
  norm_range, norm_hist, norm_trials   spk_backend.llr_range / llr_hist / llr_trials with the normalised score
                   sn(i, j) = 0.5 ((s - mu_i) r_i + (s - mu_j) r_j) in place of s (csrc/spk.hip's NormScore)
  make_cohort      the cohort rows from embeddings, on the host: the speakers' means or the rows themselves, at most max_rows
  score_all_pairs, score_trials   a back end's scores ("plda"), or the cosine of its first stage ("lda") or of the raw
                   embeddings ("cosine"), normalised: EER, threshold and min_dcf as spk_backend.Backend.score_all_pairs gives them

sn does not change under s -> alpha s + beta applied to pair and cohort scores alike, so the cosine back ends use the same kernels
on rows of unit length with a = 0 and c = 0 (the dot is then the cosine up to rounding).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import hip_ext
import spk_backend as SB

#: include/fhvae_snorm.h
SN_NAN, SN_BAD_INDEX, SN_NONFINITE = 1, 2, 4
SN_MAX_ROWS = 1 << 24
SN_MAX_COHORT = 1 << 20

_vp, _i64, _f = C.c_void_p, C.c_int64, C.c_float
#: the entry points of include/fhvae_snorm.h: name -> (restype, argtypes); bound from this table (hip_ext.load)
SN_SIGNATURES = {
    "fhvae_sn_ws_bytes": (_i64, [_i64, _i64]),
    "fhvae_sn_cohort_stats": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _f, _i64, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fhvae_sn_range": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _f, _vp, _i64, _vp, _vp, _vp]),
    "fhvae_sn_hist": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _f, _f, _f, _i64, _vp, _vp, _vp]),
    "fhvae_sn_trials": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _f, _vp, _i64, _vp, _vp, _vp]),
}

_STATUS = ((SN_NAN, "a trial's normalised score is NaN (rows or cohort statistics that are not finite?); it is counted in neither class"),
           (SN_BAD_INDEX, "a trial names a row outside the embeddings"),
           (SN_NONFINITE, "a cohort score is not finite (an evaluation or cohort row that is not finite?); that row's statistics are NaN"))
_NOUN = "score normalisation"
WHICH = ("plda", "lda", "cosine")
MODES = ("speaker-means", "rows")


def load_library():
    """hip_binding.load_library() with the entry points of include/fhvae_snorm.h bound (argtypes from SN_SIGNATURES)."""
    return hip_ext.load(SN_SIGNATURES)


def check_status(symbol, status):
    """Reads the status word (one host sync) and raises on what the kernels refused."""
    hip_ext.check_status(symbol, status, _STATUS)


# ---------------------------------------------------------------------------------------------------------------- raw calls
def _rows(op, name, t, vec_name, vec, limit):
    import torch

    t = hip_ext.device_tensor(op, name, t, _NOUN, torch.float32, 2)
    N, D = int(t.shape[0]), int(t.shape[1])
    if N < 1 or N > limit or D < 16 or D > 128 or D % 16:
        raise RuntimeError("%s: %s holds %d rows of %d columns (1 <= rows <= %d, D a multiple of 16 in [16, 128], zero-padded)" % (op, name, N, D, limit))
    if not hip_ext.rows_dense(t, D):
        t = t.contiguous()
    vec = hip_ext.device_tensor(op, vec_name, vec, _NOUN, torch.float32, 1, (N,), contiguous=True)
    return t, vec, N, D


def cohort_stats(v, a, z, az, c, top=0, sd_floor=1e-6, status=None):
    """fhvae_sn_cohort_stats: evaluation rows v (S, D) and a (S,), cohort rows z (Nc, D) and az (Nc,), f32 on the device, c a float
    -> (mu, sd, r, thr), each (S,) f32 on the device: mean and standard deviation (at least sd_floor) of the K = min(top, Nc)
    largest of s(i, n) = v_i . z_n + a_i + az_n + c over n (top <= 0: all Nc), r = 1 / sd, thr the K-th largest.  A row with a
    score that is not finite gets four NaN and sets SN_NONFINITE.  With `status` (a hip_ext.status_word) the call only enqueues
    and the caller reads the word; without, it is read here (one host sync)."""
    import torch

    import hip_binding as hb

    op = "sn_cohort_stats"
    load_library()
    v, a, S, D = _rows(op, "v", v, "a", a, SN_MAX_ROWS)
    z, az, Nc, Dz = _rows(op, "z", z, "az", az, SN_MAX_COHORT)
    if Dz != D:
        raise RuntimeError("%s: the cohort rows have %d columns, the evaluation rows %d" % (op, Dz, D))
    sd_floor = float(sd_floor)
    if not (sd_floor > 0.0 and np.isfinite(sd_floor)):
        raise RuntimeError("%s: sd_floor = %r must be positive and finite" % (op, sd_floor))
    mu, sd, r, thr = (torch.empty(S, dtype=torch.float32, device=v.device) for _ in range(4))
    own = status is None
    status = hip_ext.status_word(v.device) if own else status
    hb._call("fhvae_sn_cohort_stats", hb._p(v), v.stride(0), hb._p(a), S, hb._p(z), z.stride(0), hb._p(az), Nc, D, float(c), int(top), sd_floor,
             hb._p(mu), hb._p(sd), hb._p(r), hb._p(thr), hb._p(status))
    if own:
        check_status("fhvae_sn_cohort_stats", status)
    return mu, sd, r, thr


def _scored(op, v, a, mu, r, label=None):
    import torch

    v, a, label, S, D = SB._scored(op, v, a, label)
    mu = hip_ext.device_tensor(op, "mu", mu, _NOUN, torch.float32, 1, (S,), contiguous=True)
    r = hip_ext.device_tensor(op, "r", r, _NOUN, torch.float32, 1, (S,), contiguous=True)
    return v, a, mu, r, label, S, D


def norm_range(v, a, mu, r, label, c, status=None):
    """fhvae_sn_range: spk_backend.llr_range of the normalised score, mu and r (S,) from cohort_stats -> (2, 2) f32 device tensor."""
    import torch

    import hip_binding as hb

    op = "sn_range"
    lib = load_library()
    v, a, mu, r, label, S, D = _scored(op, v, a, mu, r, label)
    ws = hip_ext.workspace("snorm", v.device, int(lib.fhvae_sn_ws_bytes(S, D)))
    out = torch.empty(2, 2, dtype=torch.float32, device=v.device)
    own = status is None
    status = hip_ext.status_word(v.device) if own else status
    hb._call("fhvae_sn_range", hb._p(v), v.stride(0), hb._p(a), hb._p(mu), hb._p(r), hb._p(label), S, D, float(c), hb._p(ws), ws.numel(),
             hb._p(out), hb._p(status))
    if own:
        check_status("fhvae_sn_range", status)
    return out


def norm_hist(v, a, mu, r, label, c, lo, hi, n_bins=4096, status=None):
    """fhvae_sn_hist: spk_backend.llr_hist of the normalised score -> (2, n_bins) int64 device counts."""
    import torch

    import hip_binding as hb

    op = "sn_hist"
    load_library()
    v, a, mu, r, label, S, D = _scored(op, v, a, mu, r, label)
    n_bins, lo, hi = int(n_bins), float(np.float32(lo)), float(np.float32(hi))
    if n_bins < 64 or n_bins > 8192 or n_bins & (n_bins - 1):
        raise RuntimeError("%s: n_bins = %d must be a power of two in [64, 8192]" % (op, n_bins))
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
        raise RuntimeError("%s: the score range [%r, %r] must be finite and ordered" % (op, lo, hi))
    hist = torch.empty(2, n_bins, dtype=torch.int64, device=v.device)
    own = status is None
    status = hip_ext.status_word(v.device) if own else status
    hb._call("fhvae_sn_hist", hb._p(v), v.stride(0), hb._p(a), hb._p(mu), hb._p(r), hb._p(label), S, D, float(c), lo, hi, n_bins, hb._p(hist),
             hb._p(status))
    if own:
        check_status("fhvae_sn_hist", status)
    return hist


def norm_trials(v, a, mu, r, c, pairs, status=None):
    """fhvae_sn_trials: spk_backend.llr_trials of the normalised score: pairs (n, 2) int32 on the device -> (n,) f32."""
    import torch

    import hip_binding as hb

    op = "sn_trials"
    load_library()
    v, a, mu, r, _, S, D = _scored(op, v, a, mu, r)
    pairs = hip_ext.device_tensor(op, "pairs", pairs, _NOUN, torch.int32, 2, contiguous=True)
    n = int(pairs.shape[0])
    if n < 1 or int(pairs.shape[1]) != 2:
        raise RuntimeError("%s: pairs must be (n, 2) with at least one trial" % op)
    out = torch.empty(n, dtype=torch.float32, device=v.device)
    own = status is None
    status = hip_ext.status_word(v.device) if own else status
    hb._call("fhvae_sn_trials", hb._p(v), v.stride(0), hb._p(a), hb._p(mu), hb._p(r), S, D, float(c), hb._p(pairs), n, hb._p(out), hb._p(status))
    if own:
        check_status("fhvae_sn_trials", status)
    return out


# --------------------------------------------------------------------------------------------------------------------- host
def make_cohort(emb, labels=None, mode="speaker-means", max_rows=None, seed=0):
    """The cohort rows from (N, D) embeddings, on the host -> (Nc, D) f32 numpy.  "speaker-means": one row per speaker, the mean
    of its rows (labels (N,) integers, -1: the row is ignored), in increasing label; "rows": the rows themselves (the labelled
    ones where labels are given).  More than max_rows: a random subset of max_rows (RandomState(seed)), in their order."""
    x = np.asarray(emb.cpu() if hasattr(emb, "cpu") else emb, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 1:
        raise ValueError("make_cohort takes (N, D) embeddings with at least one row")
    if mode not in MODES:
        raise ValueError("mode = %r: \"speaker-means\" or \"rows\"" % (mode,))
    lab = None
    if labels is not None:
        lab = np.asarray(labels.cpu() if hasattr(labels, "cpu") else labels)
        if lab.ndim != 1 or lab.shape[0] != x.shape[0]:
            raise ValueError("make_cohort takes (N,) labels, one per row of the embeddings")
    if mode == "speaker-means":
        if lab is None:
            raise ValueError("make_cohort: the speakers' means need labels (or mode=\"rows\")")
        x, lab = x[lab >= 0], lab[lab >= 0]
        names, idx, counts = np.unique(lab, return_inverse=True, return_counts=True)
        sums = np.zeros((len(names), x.shape[1]))
        np.add.at(sums, idx, x)
        x = sums / counts[:, None]
    elif lab is not None:
        x = x[lab >= 0]
    if x.shape[0] < 1:
        raise ValueError("make_cohort: no labelled row")
    if not np.isfinite(x).all():
        raise ValueError("make_cohort: a cohort row is not finite")
    if max_rows is not None and x.shape[0] > int(max_rows):
        if int(max_rows) < 1:
            raise ValueError("make_cohort: max_rows = %r must be positive" % (max_rows,))
        x = x[np.sort(np.random.RandomState(seed).choice(x.shape[0], int(max_rows), replace=False))]
    return np.ascontiguousarray(x, dtype=np.float32)


def _unit(t):
    """(N, D) device rows -> rows of unit length (torch ops: plumbing), zero-padded to a multiple of 16, and a = 0."""
    import torch

    t = t / torch.linalg.vector_norm(t, dim=1, keepdim=True).clamp_min(1e-30)
    t = hip_ext.pad_rows(t, 16)
    if int(t.shape[1]) > 128:
        raise ValueError("score normalisation: %d columns, the kernels take at most 128" % int(t.shape[1]))
    return t, torch.zeros(int(t.shape[0]), dtype=torch.float32, device=t.device)


def operands(backend, emb, which="plda", device=None):
    """The rows a back end scores -> (v (N, Dp) f32, a (N,) f32, c) on the device.  "plda": backend.transform and its constant;
    "lda": the rows after the back end's first stage, made unit length; "cosine": the embeddings themselves, made unit length
    (the back end is not used and may be None)."""
    if which not in WHICH:
        raise ValueError("which = %r: \"plda\", \"lda\" or \"cosine\"" % (which,))
    if which == "plda":
        v, a = backend.transform(emb, device)
        return v, a, float(np.float32(backend.c))
    if which == "lda":
        K1 = int(backend.m2.shape[0])
        v, a = _unit(backend.project_lda(emb, device)[:, :K1])
    else:
        v, a = _unit(SB.Backend._rows(emb, device))
    return v, a, 0.0


def score_all_pairs(backend, emb, labels, cohort_emb, top=200, which="plda", n_bins=4096, dcf=(0.01, 1.0, 1.0), sd_floor=1e-6, device=None) -> dict:
    """Every pair i < j of labelled rows, scored, normalised against the cohort and counted on the GPU with no (S, S) and no
    (S, Nc) matrix: the statistics of each row's `top` largest cohort scores (0: the whole cohort, S-norm), the range of the
    normalised scores, their histogram over it.  -> spk_backend.eer_from_hist's dict (eer, threshold, min_dcf, crossing_mass,
    lo, hi, ...) plus "hist" (2, n_bins) int64 numpy, "top" (the K used) and "cohort" (its rows)."""
    v, a, c = operands(backend, emb, which, device)
    z, az, _ = operands(backend, cohort_emb, which, v.device)
    lab = SB.Backend._labels(labels, int(v.shape[0]), v.device)
    status = hip_ext.status_word(v.device)
    mu, _, r, _ = cohort_stats(v, a, z, az, c, top, sd_floor, status=status)
    rng = norm_range(v, a, mu, r, lab, c, status=status).cpu().numpy()
    if not np.isfinite(rng).all():
        check_status("fhvae_sn_range", status)
        for cls, what in ((0, "no target trials: no two labelled sequences share a speaker"),
                          (1, "no non-target trials: all labelled sequences have the same speaker")):
            if rng[cls, 0] > rng[cls, 1]:
                raise ValueError(what)
        raise ValueError("score_all_pairs: a normalised score is infinite")
    lo, hi = float(rng[:, 0].min()), float(rng[:, 1].max())
    hist = norm_hist(v, a, mu, r, lab, c, lo, hi, n_bins, status=status).cpu().numpy()
    check_status("fhvae_sn_hist", status)
    out = SB.eer_from_hist(hist, lo, hi, dcf)
    Nc = int(z.shape[0])
    out["hist"], out["top"], out["cohort"] = hist, (Nc if int(top) <= 0 else min(int(top), Nc)), Nc
    return out


def score_trials(backend, emb, pairs, cohort_emb, top=200, which="plda", sd_floor=1e-6, device=None):
    """pairs (n, 2) integers, rows of emb -> (n,) f32 numpy normalised scores."""
    import torch

    v, a, c = operands(backend, emb, which, device)
    z, az, _ = operands(backend, cohort_emb, which, v.device)
    p = np.asarray(pairs.cpu() if isinstance(pairs, torch.Tensor) else pairs)
    if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 1:
        raise ValueError("score_trials takes (n, 2) pairs with at least one trial")
    if (p < 0).any() or (p >= int(v.shape[0])).any():
        raise ValueError("score_trials: a trial names a row outside the %d embeddings" % int(v.shape[0]))
    mu, _, r, _ = cohort_stats(v, a, z, az, c, top, sd_floor)
    return norm_trials(v, a, mu, r, c, torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32)).to(v.device)).cpu().numpy()
