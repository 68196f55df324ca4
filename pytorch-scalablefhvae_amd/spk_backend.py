"""spk_backend.py -- the speaker back end on embeddings: centring, LDA, length normalisation and a two-covariance
PLDA trained on labelled training embeddings, then every pair of evaluation embeddings (or a trial list) scored by the PLDA
log-likelihood ratio in place of verification.py's raw cosine.

  fit              the model from (S, D) training rows and their speakers: host, float64 numpy only -> Backend
  Backend          the model and its f32 device tables: transform, score_all_pairs, score_trials, save / load (.npz)
  project, llr_range, llr_hist, llr_trials   the bindings of include/fhvae_spk.h (csrc/spk.hip)
  eer_from_hist    verification.eer_from_hist on a histogram over [lo, hi): the threshold on the score axis, min_dcf
  exact_eer        the EER of a scored trial list, by sorting, on the host

The model (this project's definitions, written out in include/fhvae_spk.h and DESIGN.md §32):
  m      the mean of the labelled training rows
  A_lda  (K1, D): with Sw / N = L L^T (Sw ridged), the top K1 eigenvectors U of L^-1 (Sb / N) L^-T; A_lda = U^T L^-1
  y      = A_lda (x - m) (or x - m without LDA), then y sqrt(K1) / max(|y|, 1e-30) with length normalisation
  PLDA   y_ci = m2 + g_c + e_ci, g ~ N(0, B), e ~ N(0, W), by EM; W = L L^T, L^-1 B L^-T = U diag(psi) U^T, A_p = U^T L^-1
  u      = A_p (y - m2);  LLR(i, j) = sum_k [p_k u_ik u_jk - q_k (u_ik^2 + u_jk^2)] + c = v_i . v_j + a_i + a_j + c
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import hip_ext
import verification as V

#: include/fhvae_spk.h
SPK_NAN, SPK_BAD_INDEX = 1, 2
SPK_MAX_IN = 1024
SPK_MAX_ROWS = 1 << 24

_vp, _i64, _f = C.c_void_p, C.c_int64, C.c_float
#: the entry points of include/fhvae_spk.h: name -> (restype, argtypes).  Exported from libfhvae_hip.so but not part of
#: include/fhvae_hip.h (ABI 12 is unchanged), so they are bound from this table (hip_ext.load) and not in hip_binding.SIGNATURES
SPK_SIGNATURES = {
    "fhvae_spk_ws_bytes": (_i64, [_i64, _i64]),
    "fhvae_spk_project": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _vp, C.c_int, _vp, _vp, _vp, _i64, _vp, _vp]),
    "fhvae_spk_llr_range": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _i64, _f, _vp, _i64, _vp, _vp, _vp]),
    "fhvae_spk_llr_hist": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _i64, _f, _f, _f, _i64, _vp, _vp, _vp]),
    "fhvae_spk_llr_trials": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _f, _vp, _i64, _vp, _vp, _vp]),
}

_STATUS = ((SPK_NAN, "a trial's score is NaN (rows that are not finite?); it is counted in neither class"),
           (SPK_BAD_INDEX, "a trial names a row outside the embeddings"))
_NOUN = "the speaker back end"


def load_library():
    """hip_binding.load_library() with the entry points of include/fhvae_spk.h bound (argtypes from SPK_SIGNATURES)."""
    return hip_ext.load(SPK_SIGNATURES)


def check_status(symbol, status):
    """Reads the status word (one host sync) and raises on what the kernels refused."""
    hip_ext.check_status(symbol, status, _STATUS)


# ---------------------------------------------------------------------------------------------------------------- raw calls
def project(x, A, mean, normalise=False, q=None, scale=None, width=None):
    """fhvae_spk_project: one stage of the transform.  x (S, Din) f32 rows, A (K, Din), mean (Din,), optional q (K,), scale (K,),
    all on the device -> out (S, width) f32 (width: K rounded up to a multiple of 16 unless given; the columns from K on are
    zeros), and a (S,) f32 with q, else None."""
    import torch

    import hip_binding as hb

    op = "spk_project"
    load_library()
    x = hip_ext.device_tensor(op, "x", x, _NOUN, torch.float32, 2)
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    S, Din = int(x.shape[0]), int(x.shape[1])
    A = hip_ext.device_tensor(op, "A", A, _NOUN, torch.float32, 2, contiguous=True)
    K = int(A.shape[0])
    if int(A.shape[1]) != Din:
        raise RuntimeError("%s: A has %d columns, the rows %d" % (op, int(A.shape[1]), Din))
    if S < 1 or not 1 <= K <= 128 or not 1 <= Din <= SPK_MAX_IN:
        raise RuntimeError("%s: %d rows of %d columns onto %d (at least one row, 1 <= K <= 128, 1 <= Din <= %d)" % (op, S, Din, K, SPK_MAX_IN))
    mean = hip_ext.device_tensor(op, "mean", mean, _NOUN, torch.float32, 1, (Din,), contiguous=True)
    q = None if q is None else hip_ext.device_tensor(op, "q", q, _NOUN, torch.float32, 1, (K,), contiguous=True)
    scale = None if scale is None else hip_ext.device_tensor(op, "scale", scale, _NOUN, torch.float32, 1, (K,), contiguous=True)
    width = (K + 15) // 16 * 16 if width is None else int(width)
    if width < K or width % 4:
        raise RuntimeError("%s: width = %d must be a multiple of 4 and at least K = %d" % (op, width, K))
    out = torch.empty(S, width, dtype=torch.float32, device=x.device)
    a = torch.empty(S, dtype=torch.float32, device=x.device) if q is not None else None
    hb._call("fhvae_spk_project", hb._p(x), x.stride(0), S, Din, hb._p(A), A.stride(0), K, hb._p(mean), int(bool(normalise)), hb._p(q),
             hb._p(scale), hb._p(out), width, hb._p(a))
    return out, a


def _scored(op, v, a, label=None):
    import torch

    v = hip_ext.device_tensor(op, "v", v, _NOUN, torch.float32, 2)
    S, D = int(v.shape[0]), int(v.shape[1])
    if S < 1 or S > SPK_MAX_ROWS or D < 16 or D > 128 or D % 16:
        raise RuntimeError("%s: v holds %d rows of %d columns (1 <= S <= 2^24, D a multiple of 16 in [16, 128]: project() pads)" % (op, S, D))
    if not hip_ext.rows_dense(v, D):
        v = v.contiguous()
    a = hip_ext.device_tensor(op, "a", a, _NOUN, torch.float32, 1, (S,), contiguous=True)
    if label is not None:
        label = hip_ext.device_tensor(op, "label", label, _NOUN, torch.int32, 1, (S,), contiguous=True)
    return v, a, label, S, D


def llr_range(v, a, label, c, status=None):
    """fhvae_spk_llr_range: v (S, D), a (S,), label (S,) int32 on the device, c a float -> (2, 2) f32 device tensor, per class
    (target, non-target) the minimum and maximum score over its trials; (+inf, -inf) for a class without one.  With `status`
    (a hip_ext.status_word) the call only enqueues and the caller reads the word; without, it is read here (one host sync)."""
    import torch

    import hip_binding as hb

    op = "spk_llr_range"
    lib = load_library()
    v, a, label, S, D = _scored(op, v, a, label)
    ws = hip_ext.workspace("spk", v.device, int(lib.fhvae_spk_ws_bytes(S, D)))
    out = torch.empty(2, 2, dtype=torch.float32, device=v.device)
    own = status is None
    status = hip_ext.status_word(v.device) if own else status
    hb._call("fhvae_spk_llr_range", hb._p(v), v.stride(0), hb._p(a), hb._p(label), S, D, float(c), hb._p(ws), ws.numel(), hb._p(out), hb._p(status))
    if own:
        check_status("fhvae_spk_llr_range", status)
    return out


def llr_hist(v, a, label, c, lo, hi, n_bins=4096, status=None):
    """fhvae_spk_llr_hist: -> (2, n_bins) int64 device counts, row 0 the target and row 1 the non-target trials, a trial in bin
    clamp(floor((s - lo) n_bins / (hi - lo)), 0, n_bins - 1) (bin 0 when hi == lo).  `status` as in llr_range()."""
    import torch

    import hip_binding as hb

    op = "spk_llr_hist"
    load_library()
    v, a, label, S, D = _scored(op, v, a, label)
    n_bins, lo, hi = int(n_bins), float(np.float32(lo)), float(np.float32(hi))
    if n_bins < 64 or n_bins > 8192 or n_bins & (n_bins - 1):
        raise RuntimeError("%s: n_bins = %d must be a power of two in [64, 8192]" % (op, n_bins))
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
        raise RuntimeError("%s: the score range [%r, %r] must be finite and ordered" % (op, lo, hi))
    hist = torch.empty(2, n_bins, dtype=torch.int64, device=v.device)  # (uint64 counts; they stay far below 2^63)
    own = status is None
    status = hip_ext.status_word(v.device) if own else status
    hb._call("fhvae_spk_llr_hist", hb._p(v), v.stride(0), hb._p(a), hb._p(label), S, D, float(c), lo, hi, n_bins, hb._p(hist), hb._p(status))
    if own:
        check_status("fhvae_spk_llr_hist", status)
    return hist


def llr_trials(v, a, c, pairs, status=None):
    """fhvae_spk_llr_trials: pairs (n, 2) int32 on the device -> (n,) f32 scores; a pair with an index outside the rows scores
    NaN and sets SPK_BAD_INDEX.  `status` as in llr_range()."""
    import torch

    import hip_binding as hb

    op = "spk_llr_trials"
    load_library()
    v, a, _, S, D = _scored(op, v, a)
    pairs = hip_ext.device_tensor(op, "pairs", pairs, _NOUN, torch.int32, 2, contiguous=True)
    n = int(pairs.shape[0])
    if n < 1 or int(pairs.shape[1]) != 2:
        raise RuntimeError("%s: pairs must be (n, 2) with at least one trial" % op)
    out = torch.empty(n, dtype=torch.float32, device=v.device)
    own = status is None
    status = hip_ext.status_word(v.device) if own else status
    hb._call("fhvae_spk_llr_trials", hb._p(v), v.stride(0), hb._p(a), S, D, float(c), hb._p(pairs), n, hb._p(out), hb._p(status))
    if own:
        check_status("fhvae_spk_llr_trials", status)
    return out


# ------------------------------------------------------------------------------------------------------------ host: figures
def eer_from_hist(hist, lo, hi, dcf=(0.01, 1.0, 1.0)) -> dict:
    """hist (2, NB) counts over [lo, hi) in NB equal bins (row 0 targets) -> verification.eer_from_hist's dict with the
    threshold mapped to the score axis, lo + (t + 1) / 2 * (hi - lo), plus lo, hi and min_dcf: with dcf = (p_target, c_miss,
    c_fa), the minimum over the NB + 1 edges of p_target c_miss FRR(k) + (1 - p_target) c_fa FAR(k), divided by
    min(p_target c_miss, (1 - p_target) c_fa) (the cost of the better of "accept all" and "reject all"), from the same
    cumulative counts as the EER."""
    out = V.eer_from_hist(hist)
    lo, hi = float(lo), float(hi)
    out["threshold"] = lo + (out["threshold"] + 1.0) / 2.0 * (hi - lo)
    out["lo"], out["hi"] = lo, hi
    p, cm, cf = (float(x) for x in dcf)
    if not 0.0 < p < 1.0 or cm <= 0.0 or cf <= 0.0:
        raise ValueError("dcf = (p_target, c_miss, c_fa) = %r: 0 < p_target < 1 and positive costs" % (dcf,))
    tar, non = [[int(x) for x in row] for row in np.asarray(hist)]
    frr = np.cumsum([0] + tar, dtype=object) / np.float64(out["n_target"])
    far = (out["n_nontarget"] - np.cumsum([0] + non, dtype=object)) / np.float64(out["n_nontarget"])
    cost = p * cm * frr.astype(np.float64) + (1.0 - p) * cf * far.astype(np.float64)
    out["min_dcf"] = float(cost.min() / min(p * cm, (1.0 - p) * cf))
    return out


def exact_eer(scores, is_target) -> dict:
    """The EER of a scored trial list by sorting: accept iff score >= threshold, the thresholds the distinct scores (and one
    above all); linear interpolation between the two thresholds around FRR = FAR -> eer, threshold, n_target, n_nontarget."""
    s = np.asarray(scores, dtype=np.float64)
    t = np.asarray(is_target, dtype=bool)
    if s.ndim != 1 or s.shape != t.shape:
        raise ValueError("exact_eer takes (n,) scores and (n,) target flags")
    if np.isnan(s).any():
        raise ValueError("exact_eer: a score is NaN")
    n_tar, n_non = int(t.sum()), int((~t).sum())
    if n_tar == 0 or n_non == 0:
        raise ValueError("exact_eer: %d target and %d non-target trials" % (n_tar, n_non))
    edges = np.unique(s)
    tar, non = np.sort(s[t]), np.sort(s[~t])
    frr = np.concatenate([np.searchsorted(tar, edges, "left"), [n_tar]]) / n_tar  # targets below the threshold
    far = np.concatenate([n_non - np.searchsorted(non, edges, "left"), [0]]) / n_non
    k = int(np.argmax(frr >= far))
    if k == 0:
        return {"eer": float(frr[0]), "threshold": float(edges[0]), "n_target": n_tar, "n_nontarget": n_non}
    d0, d1 = frr[k - 1] - far[k - 1], frr[k] - far[k]
    w = -d0 / (d1 - d0)
    thr_hi = edges[k] if k < len(edges) else edges[-1]
    return {"eer": float(frr[k - 1] + w * (frr[k] - frr[k - 1])), "threshold": float(edges[k - 1] + w * (thr_hi - edges[k - 1])),
            "n_target": n_tar, "n_nontarget": n_non}


# -------------------------------------------------------------------------------------------------------------- host: model
def _labelled(emb, labels, op):
    x = np.asarray(emb, dtype=np.float64)
    lab = np.asarray(labels)
    if x.ndim != 2 or lab.ndim != 1 or lab.shape[0] != x.shape[0]:
        raise ValueError("%s takes (S, D) embeddings and (S,) labels" % op)
    keep = lab >= 0
    x, lab = x[keep], lab[keep]
    if not np.isfinite(x).all():
        raise ValueError("%s: a labelled training row is not finite" % op)
    names, idx, counts = np.unique(lab, return_inverse=True, return_counts=True)
    if len(names) < 2:
        raise ValueError("%s: %d speaker(s) among the labelled training rows, at least 2 are needed" % (op, len(names)))
    if counts.max() < 2:
        raise ValueError("%s: no speaker has 2 or more training rows" % op)
    return x, idx, counts


def scatter(x, idx, counts):
    """-> (mean, class means (C, D), Sw = sum_c sum_i (x_i - m_c)(x_i - m_c)^T, Sb = sum_c n_c (m_c - m)(m_c - m)^T)."""
    m = x.mean(axis=0)
    sums = np.zeros((len(counts), x.shape[1]))
    np.add.at(sums, idx, x)
    mc = sums / counts[:, None]
    r = x - mc[idx]
    d = mc - m
    return m, mc, r.T @ r, (d * counts[:, None]).T @ d


def _whiten(within, between, top=None):
    """within = L L^T, L^-1 between L^-T = U diag(e) U^T, eigenvalues descending -> (A = U^T L^-1 (the top rows), e)."""
    L = np.linalg.cholesky(within)
    Li = np.linalg.solve(L, np.eye(L.shape[0]))
    M = Li @ between @ Li.T
    e, U = np.linalg.eigh((M + M.T) / 2.0)
    order = np.argsort(-e)[:top]
    return U[:, order].T @ Li, e[order]


def plda_em_step(B, W, Sw, d, counts):
    """One EM iteration of the two-covariance model: d (C, K) the class means minus m2, counts (C,), Sw the within-class scatter.
    With P_c = B^-1 + n_c W^-1: P_c^-1 = B - B (B + W / n_c)^-1 B and yhat_c = B (B + W / n_c)^-1 d_c (no inverse of B is
    formed: it may be singular).  -> (B, W) as include/fhvae_spk.h's header comment and DESIGN §32 give them."""
    Cn, N, K = len(counts), int(counts.sum()), B.shape[0]
    Bn, Wn = np.zeros((K, K)), Sw.copy()
    for n in np.unique(counts):
        sel = counts == n
        G = np.linalg.solve(B + W / n, B)      # (B + W / n)^-1 B
        Pinv = B - B @ G
        Pinv = (Pinv + Pinv.T) / 2.0
        yhat = d[sel] @ G                      # rows: d_c^T (B + W / n)^-1 B = (B (B + W / n)^-1 d_c)^T
        r = d[sel] - yhat
        Bn += sel.sum() * Pinv + yhat.T @ yhat
        Wn += n * (sel.sum() * Pinv + r.T @ r)
    return Bn / Cn, Wn / N


def fit(train_emb, train_labels, lda_dim=None, length_norm=True, plda_iters=10, ridge=1e-8):
    """The back end from (S, D) training embeddings and (S,) integer speaker labels (-1: the row is ignored) -> Backend.
    Host only, float64 numpy; the definitions are the module docstring's."""
    x, idx, counts = _labelled(train_emb, train_labels, "fit")
    N, D, Cn = x.shape[0], x.shape[1], len(counts)
    plda_iters, ridge = int(plda_iters), float(ridge)
    if plda_iters < 0 or not ridge >= 0.0:
        raise ValueError("fit: plda_iters = %d and ridge = %r must not be negative" % (plda_iters, ridge))
    m, _, Sw, Sb = scatter(x, idx, counts)
    A_lda = None
    y = x - m
    if lda_dim is not None:
        lda_dim = int(lda_dim)
        if not 1 <= lda_dim <= min(D, Cn - 1):
            raise ValueError("fit: lda_dim = %d must lie in [1, min(D, speakers - 1) = %d]" % (lda_dim, min(D, Cn - 1)))
        Sw = Sw + ridge * np.trace(Sw) / D * np.eye(D)
        A_lda, _ = _whiten(Sw / N, Sb / N, lda_dim)
        y = y @ A_lda.T
    K = y.shape[1]
    if K > 128:
        raise ValueError("fit: %d columns go into the PLDA, the kernels take at most 128 (use lda_dim)" % K)
    if length_norm:
        y = y * (np.sqrt(K) / np.maximum(np.linalg.norm(y, axis=1), 1e-30))[:, None]
    m2, mc, Sw2, Sb2 = scatter(y, idx, counts)
    W = Sw2 / N
    W = W + ridge * np.trace(W) / K * np.eye(K)  # (a within-class scatter of rank below K -- few rows -- still factors)
    B = Sb2 / Cn
    for _ in range(plda_iters):
        B, W = plda_em_step(B, W, Sw2, mc - m2, counts)
    A_p, psi = _whiten(W, B)
    return Backend(m, A_lda, bool(length_norm), m2, A_p, np.maximum(psi, 0.0))


def plda_terms(psi):
    """psi (K,) -> (p, q, c) of the closed-form LLR."""
    psi = np.asarray(psi, dtype=np.float64)
    p = psi / (2.0 * psi + 1.0)
    q = psi * psi / (2.0 * (psi + 1.0) * (2.0 * psi + 1.0))
    c = 0.5 * float(np.sum(2.0 * np.log1p(psi) - np.log1p(2.0 * psi)))
    return p, q, c


class Backend:
    """A trained back end: m (D,), A_lda (K1, D) or None, length_norm, m2 (K1,), A_p (K, K1), psi (K,), float64 numpy.  The f32
    device tables made from them are built on first use, per device."""

    def __init__(self, m, A_lda, length_norm, m2, A_p, psi):
        self.m = np.asarray(m, dtype=np.float64)
        self.A_lda = None if A_lda is None else np.asarray(A_lda, dtype=np.float64)
        self.length_norm = bool(length_norm)
        self.m2, self.A_p, self.psi = (np.asarray(t, dtype=np.float64) for t in (m2, A_p, psi))
        D = self.m.shape[0]
        K1 = D if self.A_lda is None else self.A_lda.shape[0]
        if (self.m.ndim != 1 or (self.A_lda is not None and self.A_lda.shape != (K1, D)) or self.m2.shape != (K1,)
                or self.A_p.ndim != 2 or self.A_p.shape[1] != K1 or self.psi.shape != (self.A_p.shape[0],) or (self.psi < 0).any()):
            raise ValueError("Backend: the tables' shapes do not fit together")
        self.p, self.q, self.c = plda_terms(self.psi)
        self._tables = {}

    @property
    def dim(self):
        return int(self.m.shape[0])

    # ------------------------------------------------------------------------------------------------------------- tables
    def tables_f32(self):
        """The f32 tables the kernels read, as numpy: A1 (the LDA matrix, or the identity without LDA), m, A_p, m2, q, sqrt(p),
        and c as a float."""
        A1 = np.eye(self.dim) if self.A_lda is None else self.A_lda
        f = lambda t: np.ascontiguousarray(t, dtype=np.float32)  # noqa: E731
        return {"A1": f(A1), "m": f(self.m), "A_p": f(self.A_p), "m2": f(self.m2), "q": f(self.q), "sqrt_p": f(np.sqrt(self.p)),
                "c": float(np.float32(self.c))}

    def _device_tables(self, device):
        import torch

        key = str(device)
        if key not in self._tables:
            self._tables[key] = {k: (torch.from_numpy(t).to(device) if isinstance(t, np.ndarray) else t) for k, t in self.tables_f32().items()}
        return self._tables[key]

    # ---------------------------------------------------------------------------------------------------------- transform
    @staticmethod
    def _rows(emb, device):
        import torch

        if device is None:
            device = emb.device if isinstance(emb, torch.Tensor) and emb.is_cuda else torch.device("cuda:0")
        if not isinstance(emb, torch.Tensor):
            emb = torch.from_numpy(np.array(emb, dtype=np.float32))
        e = emb.to(device=device, dtype=torch.float32)
        if e.dim() != 2 or e.shape[0] < 1:
            raise ValueError("the back end takes (S, D) embeddings with at least one row")
        return e

    def project_lda(self, emb, device=None):
        """The first stage alone: (x - m) through the LDA (the identity without it), length-normalised if the model is ->
        (S, K1 padded to a multiple of 16) f32 device rows."""
        e = self._rows(emb, device)
        if int(e.shape[1]) != self.dim:
            raise ValueError("the back end was trained on %d columns, the embeddings have %d" % (self.dim, int(e.shape[1])))
        t = self._device_tables(e.device)
        return project(e, t["A1"], t["m"], normalise=self.length_norm)[0]

    def transform(self, emb, device=None):
        """emb (S, D) (array or tensor) -> (v (S, K padded to a multiple of 16) f32, a (S,) f32) on the device: two calls of
        project(), the second one with q and sqrt(p)."""
        y = self.project_lda(emb, device)
        t = self._device_tables(y.device)
        K1 = int(self.m2.shape[0])
        return project(y[:, :K1], t["A_p"], t["m2"], normalise=False, q=t["q"], scale=t["sqrt_p"])

    # -------------------------------------------------------------------------------------------------------------- score
    @staticmethod
    def _labels(labels, S, device):
        import torch

        lab = torch.as_tensor(np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).astype(np.int32)).to(device)
        if lab.dim() != 1 or lab.shape[0] != S:
            raise ValueError("the back end takes (S,) labels, one per row of the embeddings")
        return lab

    def score_all_pairs(self, emb, labels, n_bins=4096, lo=None, hi=None, backend="plda", dcf=(0.01, 1.0, 1.0), device=None) -> dict:
        """Every pair i < j of labelled rows (label -1: the row takes part in no trial), scored on the GPU with no (S, S) matrix.
        backend "plda": the log-likelihood ratio; its histogram runs over [lo, hi), by default the smallest and largest score
        (one more pass, llr_range).  backend "lda": the cosine of the rows after the first stage (hip_binding.sv_hist), over
        [-1, 1).  -> eer_from_hist's dict plus "hist", the (2, n_bins) int64 numpy histogram."""
        import hip_binding as hb

        if backend == "lda":
            y = self.project_lda(emb, device)
            hist = hb.sv_hist(y, self._labels(labels, int(y.shape[0]), y.device), n_bins).cpu().numpy()
            lo, hi = -1.0, 1.0
        elif backend == "plda":
            v, a = self.transform(emb, device)
            lab = self._labels(labels, int(v.shape[0]), v.device)
            status = hip_ext.status_word(v.device)
            if lo is None or hi is None:
                r = llr_range(v, a, lab, self.c, status=status).cpu().numpy()
                if not np.isfinite(r).all():  # (a class without a trial reads (+inf, -inf); an infinite score is no better)
                    check_status("fhvae_spk_llr_range", status)
                    for cls, what in ((0, "no target trials: no two labelled sequences share a speaker"),
                                      (1, "no non-target trials: all labelled sequences have the same speaker")):
                        if r[cls, 0] > r[cls, 1]:
                            raise ValueError(what)
                    raise ValueError("score_all_pairs: a score is infinite")
                lo = float(r[:, 0].min()) if lo is None else lo
                hi = float(r[:, 1].max()) if hi is None else hi
            lo, hi = float(np.float32(lo)), float(np.float32(hi))
            hist = llr_hist(v, a, lab, self.c, lo, hi, n_bins, status=status).cpu().numpy()
            check_status("fhvae_spk_llr_hist", status)
        else:
            raise ValueError("backend = %r: \"lda\" or \"plda\"" % (backend,))
        out = eer_from_hist(hist, lo, hi, dcf)
        out["hist"] = hist
        return out

    def score_trials(self, emb, pairs, device=None):
        """pairs (n, 2) integers, rows of emb -> (n,) f32 numpy log-likelihood ratios (exact_eer turns them into an EER)."""
        import torch

        v, a = self.transform(emb, device)
        p = np.asarray(pairs.cpu() if isinstance(pairs, torch.Tensor) else pairs)
        if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 1:
            raise ValueError("score_trials takes (n, 2) pairs with at least one trial")
        if (p < 0).any() or (p >= int(v.shape[0])).any():
            raise ValueError("score_trials: a trial names a row outside the %d embeddings" % int(v.shape[0]))
        return llr_trials(v, a, self.c, torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32)).to(v.device)).cpu().numpy()

    # --------------------------------------------------------------------------------------------------------------- file
    def save(self, path):
        np.savez(path, m=self.m, A_lda=np.zeros((0, self.dim)) if self.A_lda is None else self.A_lda, length_norm=np.array(self.length_norm),
                 m2=self.m2, A_p=self.A_p, psi=self.psi)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            missing = [k for k in ("m", "A_lda", "length_norm", "m2", "A_p", "psi") if k not in z.files]
            if missing:
                raise ValueError("%s: no back end (missing %s)" % (path, ", ".join(missing)))
            A = z["A_lda"]
            return cls(z["m"], None if A.shape[0] == 0 else A, bool(z["length_norm"]), z["m2"], z["A_p"], z["psi"])
