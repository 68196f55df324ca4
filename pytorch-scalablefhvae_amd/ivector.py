"""ivector.py -- i-vector extraction: the speaker baseline the FHVAE papers report beside every embedding, made
from this project's own MFCC rows and UBM (gmm.py), with nothing from Kaldi.

  stats, solve     the bindings of include/fhvae_ivector.h (csrc/ivector.hip): the Baum-Welch statistics n (U, C), f (U, C, Dp) of
                   every utterance of a batch in one launch; the batched float64 factor / solve / inverse of packed (R, R) matrices
  utterance_stats  gmm.loglik / posteriors, then stats, in chunks of whole utterances: no (N, C) array for the corpus exists
  whiten           ft_c(u) = (f_c(u) - n_c(u) m_c) / s_c, a row of C Dp float64 values
  pack, unpack     the lower triangle of symmetric (R, R) matrices, p = i (i + 1) / 2 + j
  estep            L_u = I + sum_c n_c(u) M_c, b_u = Tt^T ft(u) (float64 matrix products through torch: plumbing), then solve
  fit              EM with minimum divergence -> (model, history with Q after every step)
  extract          the i-vectors of a model
  save / load      one .npz, float64

A model is a dict of float64 numpy arrays: "T" (C Dp, R) the whitened total-variability matrix, "means" and "variances" (C, D) of
the UBM it was fitted under.  The definitions are this project's, written out in include/fhvae_ivector.h; no Kaldi binary was
available to compare with.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import hip_ext

#: include/fhvae_ivector.h, FHVAE_IV_*
IV_BAD_PTR, IV_NOT_PD = 1, 2
IV_SLICE = 1024
IV_MAX_RANK = 128
IV_MAX_UTT = 1 << 22
IV_MAX_ROWS, IV_MAX_COMP = 1 << 30, 1 << 20
IV_MAX_DP = 64

_vp, _i64 = C.c_void_p, C.c_int64
#: the entry points of include/fhvae_ivector.h: name -> (restype, argtypes).  Exported from libfhvae_hip.so but not part of
#: include/fhvae_hip.h (ABI 12 is unchanged), so they are bound from this table (hip_ext.load) and not in hip_binding.SIGNATURES
IV_SIGNATURES = {
    "fhvae_iv_ws_bytes": (_i64, [_i64, _i64, _i64, _i64]),
    "fhvae_iv_stats": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "fhvae_iv_solve": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
}

_STATUS = ((IV_BAD_PTR, "an utterance's pointers decrease or leave the rows; its statistics are zeros"),
           (IV_NOT_PD, "an utterance's posterior precision is not positive definite; its results are NaN"))
_NOUN = "i-vector extraction"


def load_library():
    """hip_binding.load_library() with the entry points of include/fhvae_ivector.h bound (argtypes from IV_SIGNATURES)."""
    return hip_ext.load(IV_SIGNATURES)


def check_status(symbol, status):
    """Reads the status word (one host sync) and raises on what the kernels refused."""
    hip_ext.check_status(symbol, status, _STATUS)


def padded(width):
    """Dp: the width rounded up to a multiple of 8."""
    return (int(width) + 7) // 8 * 8


def ws_bytes(N, U, n_comp, Dp):
    """fhvae_iv_ws_bytes without the library: the (U + 1) int64 offsets and the f32 partials, each rounded up to 256 bytes."""
    items = -(-int(N) // IV_SLICE) + int(U)
    return ((int(U) + 1) * 8 + 255) // 256 * 256 + (items * int(n_comp) * (int(Dp) + 1) * 4 + 255) // 256 * 256


# ---------------------------------------------------------------------------------------------------------------- raw calls
def stats(x, post, utt_ptr, status=None):
    """fhvae_iv_stats.  x (N, D) f32, post (N, C) f32, utt_ptr (U + 1,) int64, all on the device -> (n (U, C) f32, f (U, C, Dp)
    f32): per utterance u, over its rows [utt_ptr[u], utt_ptr[u + 1]), the sums of post and of post * x (Dp: D rounded up to a
    multiple of 8; the padding columns are 0).  An utterance's result is bitwise the same alone and in any batch.  With `status`
    (a hip_ext.status_word) the call only enqueues and the caller reads the word; without, it is read here (one host sync)."""
    import torch

    import hip_binding as hb

    op = "iv_stats"
    lib = load_library()
    x, D = hip_ext.padded_rows(op, "x", x, _NOUN, 8, IV_MAX_DP, IV_MAX_ROWS)
    N, Dp = int(x.shape[0]), int(x.shape[1])
    post = hip_ext.device_tensor(op, "post", post, _NOUN, torch.float32, 2)
    n_comp = int(post.shape[1])
    if int(post.shape[0]) != N or n_comp < 1 or n_comp > IV_MAX_COMP:
        raise RuntimeError("%s: post is %s, the rows are %d (1 <= C <= %d)" % (op, tuple(post.shape), N, IV_MAX_COMP))
    if not hip_ext.rows_dense(post, n_comp):
        raise RuntimeError("%s: post needs dense rows, a row stride that is a multiple of 4 and a 16-byte aligned start (strides %s)"
                           % (op, tuple(post.stride())))
    utt_ptr = hip_ext.device_tensor(op, "utt_ptr", utt_ptr, _NOUN, torch.int64, 1, contiguous=True)
    U = int(utt_ptr.shape[0]) - 1
    if U < 1 or U > IV_MAX_UTT:
        raise RuntimeError("%s: utt_ptr holds %d entries (U + 1 with 1 <= U <= %d)" % (op, U + 1, IV_MAX_UTT))
    need = int(lib.fhvae_iv_ws_bytes(N, U, n_comp, Dp))
    if need <= 0:
        raise RuntimeError("%s: %d rows / %d utterances / %d components / %d columns lie outside the kernels' limits" % (op, N, U, n_comp, Dp))
    ws = hip_ext.workspace("ivector", x.device, need)
    n = torch.empty(U, n_comp, dtype=torch.float32, device=x.device)
    f = torch.empty(U, n_comp, Dp, dtype=torch.float32, device=x.device)
    own = status is None
    status = hip_ext.status_word(x.device) if own else status
    hb._call("fhvae_iv_stats", hb._p(x), x.stride(0), N, Dp, hb._p(post), post.stride(0), n_comp, hb._p(utt_ptr), U, hb._p(ws), ws.numel(),
             hb._p(n), hb._p(f), hb._p(status))
    if own:
        check_status("fhvae_iv_stats", status)
    return n, f


def solve(Lp, b, want_E=True, want_logdet=True, status=None):
    """fhvae_iv_solve.  Lp (U, R (R + 1) / 2) float64: the packed lower triangles of symmetric positive definite matrices, b (U, R)
    float64, on the device -> (w (U, R) = L^-1 b, E (U, P) packed = L^-1 + w w^T or None, logdet (U,) or None).  A matrix that
    is not positive definite gives NaN in its rows and sets IV_NOT_PD.  `status` as in stats(): with a word of the caller's the
    call only enqueues, and the caller decides what IV_NOT_PD means."""
    import torch

    import hip_binding as hb

    op = "iv_solve"
    load_library()
    b = hip_ext.device_tensor(op, "b", b, _NOUN, torch.float64, 2, contiguous=True)
    U, R = int(b.shape[0]), int(b.shape[1])
    if U < 1 or U > IV_MAX_UTT or R < 1 or R > IV_MAX_RANK:
        raise RuntimeError("%s: b is %s (1 <= U <= %d, 1 <= R <= %d)" % (op, tuple(b.shape), IV_MAX_UTT, IV_MAX_RANK))
    P = R * (R + 1) // 2
    Lp = hip_ext.device_tensor(op, "Lp", Lp, _NOUN, torch.float64, 2, (U, P), contiguous=True)
    w = torch.empty(U, R, dtype=torch.float64, device=b.device)
    E = torch.empty(U, P, dtype=torch.float64, device=b.device) if want_E else None
    logdet = torch.empty(U, dtype=torch.float64, device=b.device) if want_logdet else None
    own = status is None
    status = hip_ext.status_word(b.device) if own else status
    hb._call("fhvae_iv_solve", hb._p(Lp), hb._p(b), U, R, hb._p(w), hb._p(E), hb._p(logdet), hb._p(status))
    if own:
        check_status("fhvae_iv_solve", status)
    return w, E, logdet


# ------------------------------------------------------------------------------------------------------------------ triangles
def tri_index(R):
    """(rows, cols) of the packed lower triangle of an (R, R) matrix: p = i (i + 1) / 2 + j, j <= i."""
    return np.tril_indices(int(R))


def pack(S):
    """(..., R, R) symmetric -> (..., R (R + 1) / 2): the lower triangle by rows.  numpy or torch."""
    i, j = tri_index(S.shape[-1])
    out = S[..., i, j]
    return np.ascontiguousarray(out) if isinstance(out, np.ndarray) else out.contiguous()


def unpack(Sp, R):
    """The inverse of pack: (..., P) -> (..., R, R) symmetric.  numpy or torch."""
    i, j = tri_index(R)
    if Sp.shape[-1] != i.shape[0]:
        raise ValueError("unpack: %d packed values are no triangle of rank %d" % (Sp.shape[-1], R))
    if isinstance(Sp, np.ndarray):
        out = np.zeros(Sp.shape[:-1] + (R, R), dtype=Sp.dtype)
    else:
        out = Sp.new_zeros(tuple(Sp.shape[:-1]) + (R, R))
    out[..., i, j] = Sp
    out[..., j, i] = Sp
    return out


# --------------------------------------------------------------------------------------------------------------- statistics
def _ubm_arrays(op, ubm):
    try:
        w, mu, var = (np.asarray(_host(ubm[key]), dtype=np.float64) for key in ("weights", "means", "variances"))
    except (KeyError, TypeError):
        raise RuntimeError("%s: the UBM is a gmm.py model: a dict of weights, means and variances" % op) from None
    if mu.ndim != 2 or var.shape != mu.shape or w.shape != (mu.shape[0],):
        raise RuntimeError("%s: weights %s, means %s, variances %s are no (C,), (C, D), (C, D)" % (op, w.shape, mu.shape, var.shape))
    return w, mu, var


def _host(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else v


def utterance_chunks(utt_ptr, n_comp, width, max_bytes=512 << 20):
    """[(a, b)]: consecutive whole utterances a .. b - 1 per call, as many as keep the (rows, C rounded up to 4) f32 posteriors
    plus the statistics' workspace within max_bytes, and at least one.  A function of its arguments alone."""
    ptr = hip_ext.host_ptr("utterance_stats", "utt_ptr", utt_ptr)
    ldp, Dp = (int(n_comp) + 3) // 4 * 4, padded(width)
    out, a = [], 0
    U = int(ptr.shape[0]) - 1
    while a < U:
        b = a + 1
        while b < U:
            rows = int(ptr[b + 1] - ptr[a])
            if rows * ldp * 4 + ws_bytes(max(rows, 1), b + 1 - a, n_comp, Dp) > max_bytes:
                break
            b += 1
        out.append((a, b))
        a = b
    return out


def utterance_stats(rows, utt_ptr, ubm, max_bytes=512 << 20):
    """rows (N, D) f32 on the device, utterance u its rows [utt_ptr[u], utt_ptr[u + 1]) (host integers, monotone from 0), ubm a
    gmm.py model -> (n (U, C) f32, f (U, C, Dp) f32) on the device: gmm.loglik and gmm.posteriors, then stats, per chunk of
    utterance_chunks.  An utterance's statistics do not depend on its chunk."""
    import torch

    import gmm

    op = "utterance_stats"
    ptr = hip_ext.host_ptr(op, "utt_ptr", utt_ptr)
    rows = hip_ext.device_tensor(op, "rows", rows, _NOUN, torch.float32, 2)
    if int(ptr[-1]) != int(rows.shape[0]):
        raise RuntimeError("%s: utt_ptr ends at %d, the rows are %d" % (op, int(ptr[-1]), int(rows.shape[0])))
    _, mu, _ = _ubm_arrays(op, ubm)
    if mu.shape[1] != int(rows.shape[1]):
        raise RuntimeError("%s: the rows have %d columns, the UBM %d" % (op, int(rows.shape[1]), mu.shape[1]))
    tab, cst = gmm.table({k: torch.as_tensor(np.asarray(_host(v), dtype=np.float64)) for k, v in ubm.items() if k in ("weights", "means", "variances")},
                         rows.device)
    n_comp, U, Dp = int(tab.shape[0]), int(ptr.shape[0]) - 1, padded(rows.shape[1])
    x = hip_ext.pad_rows(rows, 8)
    n = torch.zeros(U, n_comp, dtype=torch.float32, device=rows.device)
    f = torch.zeros(U, n_comp, Dp, dtype=torch.float32, device=rows.device)
    status = hip_ext.status_word(rows.device)
    for a, b in utterance_chunks(ptr, n_comp, rows.shape[1], max_bytes):
        r0, r1 = int(ptr[a]), int(ptr[b])
        if r1 == r0:
            continue  # (empty utterances only: their statistics are the zeros above)
        xc = x[r0:r1]
        ll, _ = gmm.loglik(xc, tab, cst)
        post = gmm.posteriors(xc, tab, cst, ll)
        local = torch.from_numpy(ptr[a:b + 1] - ptr[a]).to(rows.device)
        n[a:b], f[a:b] = stats(xc, post, local, status=status)
    check_status("fhvae_iv_stats", status)
    return n, f


def whiten(n, f, ubm):
    """n (U, C), f (U, C, Dp) of stats() -> ft (U, C Dp) float64 on the device: (f_c - n_c m_c) / s_c in float64 torch ops, the
    padding columns 0."""
    import torch

    op = "whiten"
    n = hip_ext.device_tensor(op, "n", n, _NOUN, (torch.float32, torch.float64), 2)
    U, n_comp = int(n.shape[0]), int(n.shape[1])
    f = hip_ext.device_tensor(op, "f", f, _NOUN, (torch.float32, torch.float64), 3)
    _, mu, var = _ubm_arrays(op, ubm)
    D, Dp = mu.shape[1], padded(mu.shape[1])
    if mu.shape[0] != n_comp or tuple(f.shape) != (U, n_comp, Dp):
        raise RuntimeError("%s: n %s and f %s do not fit a UBM of %d components and %d columns (Dp = %d)"
                           % (op, tuple(n.shape), tuple(f.shape), mu.shape[0], D, Dp))
    m = torch.zeros(n_comp, Dp, dtype=torch.float64, device=n.device)
    inv = torch.zeros(n_comp, Dp, dtype=torch.float64, device=n.device)
    m[:, :D] = torch.from_numpy(mu).to(n.device)
    inv[:, :D] = 1.0 / torch.sqrt(torch.from_numpy(var).to(n.device))
    ft = (f.double() - n.double()[:, :, None] * m[None]) * inv[None]
    return ft.reshape(U, n_comp * Dp)


# ----------------------------------------------------------------------------------------------------------------------- EM
def _gram(T, n_comp, Dp):
    """M (C, P) float64 numpy: the packed T_c^T T_c, on the host."""
    R = T.shape[1]
    Tc = T.reshape(n_comp, Dp, R)
    return pack(np.matmul(Tc.transpose(0, 2, 1), Tc))


def _utt_chunk(U, R, max_bytes):
    """utterances per chunk of estep: Lp and E (U, P) and b, w (U, R) float64 within max_bytes, at least one."""
    P = R * (R + 1) // 2
    return max(1, min(int(U), int(max_bytes) // ((2 * P + 2 * R) * 8)))


def estep(n, ft, T, want_E=False, want_Q=False, max_bytes=1 << 30, each=None):
    """The E-step of the model T ((C Dp, R) float64 numpy) on the statistics n (U, C), ft (U, C Dp) float64 (whiten) on the device
    -> (w (U, R) float64, E (U, P) packed or None, Q a float or None, bad: the utterances whose precision did not factor).
    Per chunk of utterances: Lp = pack(I) + n M and b = ft T as float64 matrix products through torch, then solve.  `each(a, b,
    w, E)` is called per chunk instead of keeping E for all utterances (fit's M-step sums from it)."""
    import torch

    op = "estep"
    n = hip_ext.device_tensor(op, "n", n, _NOUN, (torch.float32, torch.float64), 2)
    ft = hip_ext.device_tensor(op, "ft", ft, _NOUN, torch.float64, 2)
    T = np.ascontiguousarray(T, dtype=np.float64)
    U, n_comp = int(n.shape[0]), int(n.shape[1])
    if T.ndim != 2 or T.shape[0] != int(ft.shape[1]) or T.shape[0] % n_comp or not 1 <= T.shape[1] <= IV_MAX_RANK or int(ft.shape[0]) != U:
        raise RuntimeError("%s: n %s, ft %s and T %s do not fit (1 <= R <= %d)" % (op, tuple(n.shape), tuple(ft.shape), T.shape, IV_MAX_RANK))
    R, Dp = T.shape[1], T.shape[0] // n_comp
    dev = n.device
    M = torch.from_numpy(_gram(T, n_comp, Dp)).to(dev)
    Td = torch.from_numpy(T).to(dev)
    eye = torch.from_numpy(pack(np.eye(R))).to(dev)
    nd = n.double()
    w = torch.empty(U, R, dtype=torch.float64, device=dev)
    E_all = torch.empty(U, R * (R + 1) // 2, dtype=torch.float64, device=dev) if want_E and each is None else None
    Q = torch.zeros((), dtype=torch.float64, device=dev)
    status = hip_ext.status_word(dev)
    step = _utt_chunk(U, R, max_bytes)
    for a in range(0, U, step):
        b = min(U, a + step)
        Lp = (nd[a:b] @ M + eye[None]).contiguous()
        bu = (ft[a:b] @ Td).contiguous()
        wc, Ec, ld = solve(Lp, bu, want_E=want_E, want_logdet=want_Q, status=status)
        w[a:b] = wc
        if want_Q:
            Q = Q + (-0.5 * ld + 0.5 * (bu * wc).sum(dim=1)).sum()
        if each is not None:
            each(a, b, wc, Ec)
        elif E_all is not None:
            E_all[a:b] = Ec
    st = int(status.item())
    bad = int(torch.isnan(w[:, 0]).sum()) if st & IV_NOT_PD else 0
    return w, E_all, (float(Q) if want_Q else None), bad


def _mstep(n, ft, T, n_comp, Dp, max_bytes):
    """One E-step with its sums -> (T_new, Q of T, the mean of E packed, bad)."""
    import torch

    R = T.shape[1]
    P = R * (R + 1) // 2
    dev = n.device
    A = torch.zeros(n_comp, P, dtype=torch.float64, device=dev)
    K = torch.zeros(n_comp * Dp, R, dtype=torch.float64, device=dev)
    Esum = torch.zeros(P, dtype=torch.float64, device=dev)
    nd = n.double()

    def each(a, b, wc, Ec):
        A.add_(nd[a:b].t() @ Ec)
        K.add_(ft[a:b].t() @ wc)
        Esum.add_(Ec.sum(dim=0))

    _, _, Q, bad = estep(n, ft, T, want_E=True, want_Q=True, max_bytes=max_bytes, each=each)
    if bad:
        raise ValueError("fit: %d utterances' posterior precisions did not factor" % bad)
    Ah = unpack(A.cpu().numpy(), R)
    Kh = K.cpu().numpy().reshape(n_comp, Dp, R)
    Tn = np.empty_like(Kh)
    for c in range(n_comp):  # T_c A_c = K_c, A_c symmetric: C solves on the host in float64
        Tn[c] = np.linalg.solve(Ah[c], Kh[c].T).T
    return Tn.reshape(n_comp * Dp, R), Q, Esum.cpu().numpy() / float(n.shape[0])


def fit(n, f, ubm, rank, iters=10, seed=0, min_div=True, max_bytes=1 << 30):
    """EM for the total-variability matrix on the statistics n (U, C), f (U, C, Dp) of utterance_stats under `ubm`.

    The start is 0.1 times standard normal draws of numpy.random.default_rng(seed), shape (C Dp, R), with the rows of the padding
    columns 0.  An iteration is an E-step, the M-step T_c <- K_c A_c^-1 and, with min_div, a second E-step with the new T, P = mean
    E = G G^T and T <- T G.  A component no utterance has any posterior mass for (A_c singular) is an error.

    -> (model {"T", "means", "variances"}, history {"Q": the objective after the start and after every step, "steps": their names
    ("init", "m", "md", ...), "iterations"}).  Same statistics and seed: the same bits."""
    import torch  # noqa: F401

    _, mu, var = _ubm_arrays("fit", ubm)
    n_comp, D = mu.shape
    Dp, R = padded(D), int(rank)
    if not 1 <= R <= IV_MAX_RANK:
        raise ValueError("fit: rank = %d must lie in [1, %d]" % (R, IV_MAX_RANK))
    if iters < 1:
        raise ValueError("fit: iters = %d must be at least 1" % iters)
    ft = whiten(n, f, ubm)
    rng = np.random.default_rng(int(seed))
    T = np.zeros((n_comp, Dp, R))
    T[:, :D, :] = 0.1 * rng.standard_normal((n_comp, D, R))
    T = T.reshape(n_comp * Dp, R)
    hist = {"Q": [], "steps": [], "iterations": 0}

    def record(name, q):
        hist["steps"].append(name), hist["Q"].append(q)

    name = "init"
    for it in range(1, int(iters) + 1):
        T, q, _ = _mstep(n, ft, T, n_comp, Dp, max_bytes)
        record(name, q)  # (the E-step's Q belongs to the model it was run on: the step before)
        name = "m"
        if min_div:
            _, q, Emean = _md_estep(n, ft, T, max_bytes)
            record("m", q)
            T = T @ np.linalg.cholesky(unpack(Emean, R))
            name = "md"
        hist["iterations"] = it
    _, _, q, bad = estep(n, ft, T, want_Q=True, max_bytes=max_bytes)
    if bad:
        raise ValueError("fit: %d utterances' posterior precisions did not factor" % bad)
    record(name, q)
    return {"T": T, "means": mu, "variances": var}, hist


def _md_estep(n, ft, T, max_bytes):
    import torch

    R = T.shape[1]
    Esum = torch.zeros(R * (R + 1) // 2, dtype=torch.float64, device=n.device)
    w, _, Q, bad = estep(n, ft, T, want_E=True, want_Q=True, max_bytes=max_bytes, each=lambda a, b, wc, Ec: Esum.add_(Ec.sum(dim=0)))
    if bad:
        raise ValueError("fit: %d utterances' posterior precisions did not factor" % bad)
    return w, Q, Esum.cpu().numpy() / float(n.shape[0])


def extract(n, f, model, max_bytes=1 << 30, with_bad=False):
    """The i-vectors w (U, R) float64 on the device of the statistics n, f under `model` (fit's, or load's).  with_bad: -> (w,
    the number of utterances whose precision did not factor: their rows are NaN)."""
    ft = whiten(n, f, {"weights": np.ones(model["means"].shape[0]), "means": model["means"], "variances": model["variances"]})
    w, _, _, bad = estep(n, ft, model["T"], max_bytes=max_bytes)
    return (w, bad) if with_bad else w


# --------------------------------------------------------------------------------------------------------------------- files
_KEYS = ("T", "means", "variances")


def save(path, model):
    """One .npz with T (C Dp, R), means (C, D), variances (C, D), float64."""
    arrays = {key: np.ascontiguousarray(_host(model[key]), dtype=np.float64) for key in _KEYS}
    with open(path, "wb") as fh:  # (np.savez would add ".npz" to a name without it)
        np.savez(fh, **arrays)


def load(path):
    """The inverse of save: a model of numpy float64 arrays, its shapes checked."""
    with np.load(path) as z:
        try:
            model = {key: np.asarray(z[key], dtype=np.float64) for key in _KEYS}
        except KeyError as e:
            raise ValueError("%s holds no %s: not a file ivector.save wrote" % (path, e)) from None
    T, mu, var = model["T"], model["means"], model["variances"]
    if T.ndim != 2 or mu.ndim != 2 or var.shape != mu.shape or T.shape[0] != mu.shape[0] * padded(mu.shape[1]) or not 1 <= T.shape[1] <= IV_MAX_RANK:
        raise ValueError("%s: T %s, means %s, variances %s are no (C Dp, R), (C, D), (C, D)" % (path, T.shape, mu.shape, var.shape))
    return model
