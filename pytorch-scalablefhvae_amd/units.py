"""units.py -- discrete acoustic units from frame-level representations ("Units"): a k-means codebook fitted on the
rows of a corpus, one unit per frame, and the numbers unit-discovery work reports against a phone alignment.

  assign, update   the bindings of include/fhvae_kmeans.h (csrc/kmeans.hip): nearest centroid of every row; centroid means
  fit              Lloyd's algorithm on those two, with a fixed rule for empty clusters
  frame_phones     item lines (abx.read_items) -> a phone id per frame of a corpus
  unit_quality     cluster purity, phone purity and PNMI from the (units, phones) contingency table
  bitrate          the ZeroSpeech 2019 bitrate of unit sequences, frame-level and run-length collapsed
  write_units / read_units   the text format, one line `key u0 u1 ...` per utterance
  corpus_rows, discover      what discover_units.py and eval_model.py --units run

The definitions (scores, ties, the update's summation order, the empty-cluster rule, the metrics) are this project's, written
out in include/fhvae_kmeans.h and below; nothing here runs scikit-learn or faiss.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import hip_ext

#: the bits of fhvae_km_update's int32 device status word and the limits (include/fhvae_kmeans.h, FHVAE_KM_*)
KM_BAD_PTR, KM_BAD_PERM = 1, 2
KM_PIECE = 256
KM_MAX_ROWS, KM_MAX_CENT = 1 << 30, 1 << 20
KM_MAX_DIM = 128  # (csrc/allpairs_f32.h: D a multiple of 16 in [16, 128])

_vp, _i64 = C.c_void_p, C.c_int64
#: the entry points of include/fhvae_kmeans.h: name -> (restype, argtypes).  Exported from libfhvae_hip.so but not part of
#: include/fhvae_hip.h (ABI 12 is unchanged), so they are bound from this table (hip_ext.load) and not in hip_binding.SIGNATURES
KM_SIGNATURES = {
    "fhvae_km_ws_bytes": (_i64, [_i64, _i64, _i64]),
    "fhvae_km_assign": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp]),
    "fhvae_km_update": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
}


def load_library():
    """hip_binding.load_library() with the k-means entry points bound (argtypes from KM_SIGNATURES)."""
    return hip_ext.load(KM_SIGNATURES)


# ---------------------------------------------------------------------------------------------------------------- raw calls
def _rows(op, name, t, width=None):
    """The (rows, D) f32 matrix of a k-means call: a device tensor whose rows are dense, a leading dimension that is a multiple
    of 4 and a 16-byte aligned start (views with a row stride pass as they are)."""
    import torch

    if t is None or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < 1:
        raise RuntimeError("%s: %s must be a 2-D float32 device tensor with at least one row" % (op, name))
    D = int(t.shape[1])
    if D < 16 or D > KM_MAX_DIM or D % 16 or (width is not None and D != width):
        raise ValueError("%s: %s has %d columns; the kernels take a multiple of 16 in [16, %d]%s"
                         % (op, name, D, KM_MAX_DIM, "" if width is None else ", here %d" % width))
    if not hip_ext.rows_dense(t, D):
        raise RuntimeError("%s: %s needs dense rows, a row stride that is a multiple of 4 and a 16-byte aligned start "
                           "(strides %s)" % (op, name, tuple(t.stride())))
    return t


def _workspace(dev, N, K, D):
    need = int(load_library().fhvae_km_ws_bytes(N, K, D))
    if need <= 0:
        raise ValueError("k-means: %d rows / %d centroids / %d columns lie outside the kernels' limits (%d rows, %d centroids)"
                         % (N, K, D, KM_MAX_ROWS, KM_MAX_CENT))
    return hip_ext.workspace("units", dev, need)


def assign(x, cent, want_dist=True):
    """fhvae_km_assign.  x (N, D), cent (K, D) f32 on the device -> (labels (N,) int32, dist (N,) f32 or None): every row's
    nearest centroid (equal scores: the smallest index) and its squared distance to it.  Only enqueues."""
    import torch

    import hip_binding as hb

    load_library()
    _rows("km_assign", "x", x)
    _rows("km_assign", "cent", cent, int(x.shape[1]))
    N, D, K = int(x.shape[0]), int(x.shape[1]), int(cent.shape[0])
    ws = _workspace(x.device, N, K, D)
    labels = torch.empty(N, dtype=torch.int32, device=x.device)
    dist = torch.empty(N, dtype=torch.float32, device=x.device) if want_dist else None
    hb._call("fhvae_km_assign", hb._p(x), x.stride(0), N, D, hb._p(cent), cent.stride(0), K, hb._p(ws), ws.numel(), hb._p(labels),
             hb._p(dist))
    return labels, dist


def update_members(x, perm, cl_ptr, cent, status, dist=None):
    """fhvae_km_update on the caller's member lists: perm (N,) int64, cl_ptr (K + 1,) int64, status (1,) int32, all on the device.
    cent (K, D) is updated in place.  -> (count (K,) int64, cl_inertia (K,) float64).  Only enqueues: read `status` afterwards."""
    import torch

    import hip_binding as hb

    load_library()
    _rows("km_update", "x", x)
    _rows("km_update", "cent", cent, int(x.shape[1]))
    N, D, K = int(x.shape[0]), int(x.shape[1]), int(cent.shape[0])
    hb._need_gpu(perm, cl_ptr, dist, status)
    hb._want("km_update", "perm", perm, torch.int64, shape=(N,))
    hb._want("km_update", "cl_ptr", cl_ptr, torch.int64, shape=(K + 1,))
    hb._want("km_update", "dist", dist, torch.float32, shape=(N,), optional=True)
    hb._want("km_update", "status", status, torch.int32, numel=1)
    ws = _workspace(x.device, N, K, D)
    count = torch.zeros(K, dtype=torch.int64, device=x.device)
    cl_inertia = torch.zeros(K, dtype=torch.float64, device=x.device)
    hb._call("fhvae_km_update", hb._p(x), x.stride(0), N, D, hb._p(perm), hb._p(cl_ptr), K, hb._p(dist), hb._p(ws), ws.numel(),
             hb._p(cent), cent.stride(0), hb._p(count), hb._p(cl_inertia), hb._p(status))
    return count, cl_inertia


def members(labels, K):
    """labels (N,) int32 on the device -> (perm, cl_ptr): the rows sorted by label, every cluster's rows in increasing index (a
    stable sort), and the clusters' offsets into them.  No host sync.  A label outside [0, K) leaves cl_ptr short of [0, N]:
    fhvae_km_update refuses it (KM_BAD_PTR)."""
    import torch

    ordered, perm = torch.sort(labels, stable=True)
    cl_ptr = torch.searchsorted(ordered, torch.arange(K + 1, dtype=labels.dtype, device=labels.device))
    return perm, cl_ptr


def check_status(status):
    """Reads the status word (one host sync) and raises on what the kernels refused."""
    hip_ext.check_status("fhvae_km_update", status, ((KM_BAD_PTR, "cl_ptr is not monotone from 0 to N (a label outside [0, K)?)"),
                                                    (KM_BAD_PERM, "a perm entry lies outside [0, N)")))


def update(x, labels, cent, dist=None):
    """The centroid update for `labels` (N,) int32 on the device: cent (K, D) becomes, in place, the mean of every cluster's rows
    (include/fhvae_kmeans.h: two-level float64 sums in row order; a cluster without rows keeps its centroid).  -> (count (K,)
    int64, cl_inertia (K,) float64: the clusters' sums of dist, 0 without dist).  One host sync, for the status word."""
    perm, cl_ptr = members(labels, int(cent.shape[0]))
    status = hip_ext.status_word(x.device)
    out = update_members(x, perm, cl_ptr, cent, status, dist)
    check_status(status)
    return out


# -------------------------------------------------------------------------------------------------------------------- Lloyd
def initial_rows(N, k, seed):
    """The rows whose copies are the first centroids of the restart with this seed."""
    return np.random.RandomState(seed).choice(N, k, replace=False)


def reseed(labels, dist, counts):
    """The rule for empty clusters, on the device, in place: with e clusters empty, the e rows of largest dist (equal ones: the
    smaller row index first -- a stable descending sort) go to them, in increasing k.  -> e."""
    import torch

    empty = torch.nonzero(counts == 0).flatten()
    e = int(empty.numel())
    if e:
        far = torch.sort(dist, descending=True, stable=True).indices[:e]
        labels[far] = empty.to(labels.dtype)
    return e


def _lloyd(x, cent, iters, tol):
    K = int(cent.shape[0])
    prev, prev_inertia, reseeded, converged = None, None, 0, False
    for it in range(1, iters + 1):
        labels, dist = assign(x, cent)
        perm, cl_ptr = members(labels, K)
        if int((cl_ptr[1:] == cl_ptr[:-1]).sum()):
            reseed(labels, dist, cl_ptr[1:] - cl_ptr[:-1])
            reseeded += 1
            perm, cl_ptr = members(labels, K)
        changed = True if prev is None else bool((labels != prev).any())
        status = hip_ext.status_word(x.device)
        counts, cl_inertia = update_members(x, perm, cl_ptr, cent, status, dist)
        inertia = float(np.sum(cl_inertia.cpu().numpy(), dtype=np.float64))
        check_status(status)
        if not changed:
            converged = True
        elif prev_inertia is not None and prev_inertia - inertia < tol * prev_inertia:
            converged = True
        prev, prev_inertia = labels, inertia
        if converged:
            break
    return {"centroids": cent, "labels": prev, "counts": counts, "inertia": prev_inertia, "iterations": it, "converged": converged,
            "reseeded": reseeded}


def fit(x, k, iters=100, tol=1e-4, n_init=1, seed=0, init=None):
    """Lloyd's algorithm on the rows of x ((N, D) f32 on the device).

    The first centroids are `init` ((k, D), one run) or, for restart r of n_init, the rows initial_rows(N, k, seed + r).  An
    iteration assigns every row (assign), hands the rows of largest dist to the clusters that came out empty (reseed; the rows
    are relabelled before the update and the iteration is counted in "reseeded"; a cluster a relabelled row was the only
    member of stays empty for this iteration and keeps its centroid) and updates the centroids (update).  The iteration's
    inertia is the host float64 sum of the update's cl_inertia: the rows' squared distances to the centroids they were
    assigned to.  It stops when no label differs from the iteration before, when the inertia fell by less than tol times the
    one before, or after `iters` iterations; the restart with the lowest inertia wins (the first of equal ones).  Same input
    and seed: the same bits.

    -> {"centroids" (k, D) f32 and "labels" (N,) int32 on the device; "counts" (k,) int64 numpy; "inertia"; "iterations";
    "converged"; "reseeded"}: labels, counts and inertia are the last iteration's assignment, centroids the means of it."""
    import torch

    _rows("fit", "x", x)
    N, D, k = int(x.shape[0]), int(x.shape[1]), int(k)
    if k < 1 or k > N:
        raise ValueError("fit: k = %d must lie in [1, N = %d]" % (k, N))
    if k > KM_MAX_CENT or N > KM_MAX_ROWS:
        raise ValueError("fit: at most %d rows and %d centroids" % (KM_MAX_ROWS, KM_MAX_CENT))
    if iters < 1 or n_init < 1:
        raise ValueError("fit: iters = %d and n_init = %d must be at least 1" % (iters, n_init))
    if not bool(torch.isfinite(x).all()):
        raise ValueError("fit: x holds values that are not finite")
    starts = []
    if init is not None:
        init = torch.as_tensor(init, dtype=torch.float32).to(x.device)
        if tuple(init.shape) != (k, D):
            raise ValueError("fit: init is %s, not (%d, %d)" % (tuple(init.shape), k, D))
        if not bool(torch.isfinite(init).all()):
            raise ValueError("fit: init holds values that are not finite")
        starts.append(init.clone().contiguous())
    else:
        for r in range(n_init):
            rows = torch.from_numpy(initial_rows(N, k, seed + r).astype(np.int64)).to(x.device)
            starts.append(x[rows].contiguous())
    best = None
    for cent in starts:
        res = _lloyd(x, cent, int(iters), float(tol))
        if best is None or res["inertia"] < best["inertia"]:
            best = res
    best["counts"] = best["counts"].cpu().numpy()
    return best


# ------------------------------------------------------------------------------------------------------------------ phones
def frame_phones(items, keys, lengths, frame_shift=0.010, frame_offset=0.0):
    """Item lines (abx.read_items) -> a phone per frame of a corpus whose utterances `keys` have `lengths` frames and lie one after
    the other (frames.FramePool's layout).  A token's frames are abx.frame_range's; a token of an utterance that is not in
    `keys`, or without a frame, labels nothing.  No cap on a token's length and none per cell.  Returns (phones, names,
    overlaps): phones (total frames,) int32, an index into `names` (in order of first use) or -1 where no token lies;
    overlaps, the frames a later token would have labelled again (the first token in file order keeps them)."""
    import abx

    if not frame_shift > 0:
        raise ValueError("frame_shift %g must be positive" % frame_shift)
    index = {k: i for i, k in enumerate(keys)}
    lengths = np.asarray(lengths, dtype=np.int64)
    base = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    phones = np.full(int(base[-1]), -1, dtype=np.int32)
    table, names, overlaps = {}, [], 0
    for name, on, off, phone, _, _, _ in items:
        u = index.get(name)
        if u is None:
            continue
        first, count = abx.frame_range(on, off, lengths[u], frame_shift, frame_offset)
        if count == 0:
            continue
        if phone not in table:
            table[phone] = len(names)
            names.append(phone)
        seg = phones[base[u] + first:base[u] + first + count]
        free = seg < 0
        overlaps += int(count - free.sum())
        seg[free] = table[phone]
    return phones, names, overlaps


def unit_quality(labels, phones, k, n_phones=None):
    """The (k, P) contingency table n_kp of the frames with phones >= 0, in float64, and from it
      cluster_purity = sum_k max_p n_kp / n     phone_purity = sum_p max_k n_kp / n
      pnmi = I(unit; phone) / H(phone), 0 when H(phone) = 0     labelled_frames = n
    (natural logarithms; the ratio has no unit).  Without a labelled frame the three are 0."""
    labels, phones = np.asarray(labels).astype(np.int64), np.asarray(phones).astype(np.int64)
    if labels.shape != phones.shape:
        raise ValueError("unit_quality: %d labels for %d frames" % (labels.shape[0], phones.shape[0]))
    keep = phones >= 0
    P = int(n_phones) if n_phones is not None else (int(phones.max()) + 1 if keep.any() else 0)
    table = np.zeros((int(k), max(P, 1)), dtype=np.float64)
    np.add.at(table, (labels[keep], phones[keep]), 1.0)
    n = float(table.sum())
    if n == 0:
        return {"cluster_purity": 0.0, "phone_purity": 0.0, "pnmi": 0.0, "labelled_frames": 0}
    nk, npp = table.sum(axis=1, keepdims=True), table.sum(axis=0, keepdims=True)
    nz = table > 0
    # (from the counts, which are exact: a unit that holds all of a phone and nothing else contributes log(n / n_p) exactly)
    mi = float(np.sum(table[nz] / n * np.log((table * n)[nz] / (nk * npp)[nz])))
    col = npp[npp > 0]
    hp = float(-np.sum(col / n * np.log(col / n)))
    return {"cluster_purity": float(table.max(axis=1).sum() / n), "phone_purity": float(table.max(axis=0).sum() / n),
            "pnmi": mi / hp if hp > 0 else 0.0, "labelled_frames": int(n)}


# ----------------------------------------------------------------------------------------------------------------- sequences
def collapse(seq):
    """Run-length collapse: every run of equal units becomes one."""
    seq = np.asarray(seq)
    if seq.shape[0] == 0:
        return seq
    return seq[np.concatenate([[True], seq[1:] != seq[:-1]])]


def _bits(seqs, duration):
    flat = np.concatenate([np.asarray(s, dtype=np.int64) for s in seqs]) if len(seqs) else np.zeros(0, np.int64)
    if flat.shape[0] == 0 or not duration > 0:
        return 0.0
    c = np.bincount(flat).astype(np.float64)
    p = c[c > 0] / flat.shape[0]
    return float(flat.shape[0] * -np.sum(p * np.log2(p)) / duration)


def bitrate(seqs, frame_shift=0.010):
    """The ZeroSpeech 2019 bitrate M H / duration of unit sequences (one per utterance, one unit per frame): M symbols, H the
    entropy in bits of their unigram distribution over the whole set, duration = frames * frame_shift seconds.  -> {"bitrate":
    of the sequences as they are, "bitrate_collapsed": of their run-length collapsed forms, over the same duration}."""
    duration = sum(len(s) for s in seqs) * float(frame_shift)
    return {"bitrate": _bits(seqs, duration), "bitrate_collapsed": _bits([collapse(s) for s in seqs], duration)}


def write_units(path, keys, seqs):
    """One line `key u0 u1 ...` per utterance, in the order given."""
    keys = list(keys)
    if len(keys) != len(seqs):
        raise ValueError("%d keys for %d sequences" % (len(keys), len(seqs)))
    with open(path, "w") as fh:
        for key, s in zip(keys, seqs):
            fh.write(" ".join([str(key)] + ["%d" % u for u in s]) + "\n")


def read_units(path):
    """The inverse of write_units: (keys, [int32 arrays])."""
    keys, seqs = [], []
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            f = line.split()
            if not f:
                continue
            try:
                seqs.append(np.asarray([int(u) for u in f[1:]], dtype=np.int32))
            except ValueError:
                raise ValueError("%s line %d: a unit is not an integer" % (path, no)) from None
            keys.append(f[0])
    return keys, seqs


# --------------------------------------------------------------------------------------------------------------- the corpus
def corpus_rows(model, pool, on, batch_size=16384):
    """The (total frames, D) rows of a shift-1 frames.FramePool that units are found on: "z1", frames.encode_frames' frame-level
    z1; "feats", the normalised input.  A width that is no multiple of 16 is zero-padded to the next one on the device (every
    distance is unchanged); one above KM_MAX_DIM raises ValueError.  -> (rows, width before padding)."""
    import torch

    import frames

    rows = frames.corpus_rows(model, pool, on, "units", batch_size)
    width = int(rows.shape[1])
    if width > KM_MAX_DIM:
        raise ValueError("%s has %d values per frame, the k-means kernels take at most %d" % (on, width, KM_MAX_DIM))
    if width % 16:
        rows = torch.nn.functional.pad(rows, (0, 16 - width % 16))
    return rows.contiguous(), width


def discover(rows, width, keys, lengths, on, k=None, codebook=None, iters=100, tol=1e-4, n_init=1, seed=0, items=None,
             frame_shift=0.010, frame_offset=0.0):
    """Units for the rows of a corpus (corpus_rows): fit a codebook of k centroids, or apply `codebook` ((K, width) numpy).
    -> (info, centroids (K, width) f32 numpy, counts (K,) int64 numpy, seqs: one int32 array per utterance).  info is what
    units.json holds: on, k, frames, iterations, converged, inertia, reseeded, seed, bitrate, bitrate_collapsed and, with
    `items`, unit_quality's numbers, overlaps and phones.  The units, the counts and the inertia are those of one more assignment,
    to the centroids returned (after fit's last update), so applying the written codebook to the same rows gives the same units."""
    import torch

    N = int(rows.shape[0])
    if int(np.sum(lengths)) != N:
        raise ValueError("%d rows for utterances of %d frames" % (N, int(np.sum(lengths))))
    if not bool(torch.isfinite(rows).all()):
        raise ValueError("%s holds values that are not finite" % on)
    if codebook is None:
        res = fit(rows, k, iters=iters, tol=tol, n_init=n_init, seed=seed)
        cent = res["centroids"]
        info = {"on": on, "k": int(k), "frames": N, "iterations": res["iterations"], "converged": res["converged"]}
        reseeded = res["reseeded"]
    else:
        codebook = np.asarray(codebook, dtype=np.float32)
        if codebook.ndim != 2 or codebook.shape[1] != width:
            raise ValueError("the codebook is %s, but %s has %d values per frame" % (tuple(codebook.shape), on, width))
        if not np.isfinite(codebook).all():
            raise ValueError("the codebook holds values that are not finite")
        cent = torch.nn.functional.pad(torch.from_numpy(codebook).to(rows.device), (0, int(rows.shape[1]) - width)).contiguous()
        info = {"on": on, "k": int(cent.shape[0]), "frames": N, "iterations": 0, "converged": True}
        reseeded = 0
    # the units are the rows' assignment to the centroids that are written: what --codebook with them gives again
    labels, dist = assign(rows, cent)
    counts = torch.bincount(labels.long(), minlength=int(cent.shape[0])).cpu().numpy().astype(np.int64)
    info.update({"inertia": float(dist.double().sum()), "reseeded": reseeded, "seed": int(seed)})
    host = labels.cpu().numpy()
    ptr = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])
    seqs = [host[int(a):int(b)] for a, b in zip(ptr[:-1], ptr[1:])]
    info.update(bitrate(seqs, frame_shift))
    if items is not None:
        phones, names, overlaps = frame_phones(items, keys, lengths, frame_shift, frame_offset)
        info.update(unit_quality(host, phones, info["k"], len(names)))
        info.update({"overlaps": overlaps, "phones": names})
    return info, cent[:, :width].cpu().numpy(), counts, seqs
