"""abx.py -- ABX phone discriminability of frame-level representations ("ABX"): is a token X of phone p closer, under
DTW, to another token A of p than to a token B of phone q in the same context?  Asked within one speaker and across speakers.

  dtw              the binding of include/fhvae_abx.h (csrc/abx.hip): the DTW distance between every two tokens of every group
  read_items       the ZeroSpeech / ABXpy .item text format
  tokens_from_items  item lines -> tokens on the frames of a corpus (what dtw and abx_scores work on)
  pair_distances   groups the tokens by context and yields every group's (n, n) distance block, chunked to a memory limit
  abx_scores       the within- and across-speaker error from those blocks

The definitions (frame cost, recursion, normalisation, the score's averaging) are this project's, written out in
include/fhvae_abx.h and below; nothing here runs ABXpy.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import hip_ext

#: metric of fhvae_abx_dtw, the bits of its int32 device status word and its limits (include/fhvae_abx.h, FHVAE_ABX_*)
ABX_ANGULAR, ABX_COSINE = 0, 1
ABX_BAD_TOKEN, ABX_BAD_PTR = 1, 2
ABX_MAX_DIM, ABX_MAX_LEN = 128, 64
METRICS = {"angular": ABX_ANGULAR, "cosine": ABX_COSINE}

_vp, _i64 = C.c_void_p, C.c_int64
#: the entry point of include/fhvae_abx.h: name -> (restype, argtypes).  Exported from libfhvae_hip.so but not part of
#: include/fhvae_hip.h (ABI 12 is unchanged), so it is bound from this table (hip_ext.load) and not in hip_binding.SIGNATURES
ABX_SIGNATURES = {
    "fhvae_abx_dtw": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _i64, C.c_int, _vp, _vp, _vp]),
}

#: the messages of the status bits, in the order they are named (hip_ext.check_status)
STATUS_BITS = ((ABX_BAD_TOKEN, "a token lies outside the features or is longer than %d frames" % ABX_MAX_LEN),
               (ABX_BAD_PTR, "grp_ptr / out_ptr / pair_ptr are inconsistent"))

ITEM_HEADER = "#file onset offset #phone prev-phone next-phone speaker"
#: times are compared with the frame grid to this many frames: 0.10 s is frame 10 of a 10 ms grid although 0.10 / 0.01 > 10
FRAME_EPS = 1e-6
DROP_REASONS = ("unknown_utterance", "no_frames", "too_long", "over_cell_cap")


def load_library():
    """hip_binding.load_library() with the ABX entry point bound (argtypes from ABX_SIGNATURES)."""
    return hip_ext.load(ABX_SIGNATURES)


def group_ptrs(grp_ptr):
    """grp_ptr (G + 1,) -> (out_ptr, pair_ptr): the offsets of every group's n^2 block and of its n (n - 1) / 2 pairs."""
    n = np.diff(np.asarray(grp_ptr, dtype=np.int64))
    zero = np.zeros(1, dtype=np.int64)
    return np.concatenate([zero, np.cumsum(n * n)]), np.concatenate([zero, np.cumsum(n * (n - 1) // 2)])


def dtw(feats, tok_start, tok_len, grp_ptr, metric, status, out_ptr=None, pair_ptr=None, out=None, max_len=ABX_MAX_LEN):
    """fhvae_abx_dtw.  feats (n_frames, D) f32, tok_start (N,) int64, tok_len (N,) int32 and status (1,) int32 on the device;
    grp_ptr (G + 1,) host integers (out_ptr / pair_ptr follow from it unless given).  -> out (out_ptr[-1],) f32 on the device,
    group g's (n_g, n_g) block at out_ptr[g]; a given `out` is written into.  max_len: the caller's bound on tok_len (a smaller one
    runs faster, the values are the same).  Only enqueues: read `status` afterwards."""
    import torch

    import hip_binding as hb

    load_library()
    hb._need_gpu(feats, tok_start, tok_len, status, out)
    hb._want("abx_dtw", "feats", feats, torch.float32, shape=(None, None))
    hb._want("abx_dtw", "tok_start", tok_start, torch.int64)
    hb._want("abx_dtw", "tok_len", tok_len, torch.int32, shape=tuple(tok_start.shape))
    hb._want("abx_dtw", "status", status, torch.int32, contiguous=False)
    grp_ptr = np.ascontiguousarray(grp_ptr, dtype=np.int64)
    d_out, d_pair = group_ptrs(grp_ptr)
    out_ptr = d_out if out_ptr is None else np.ascontiguousarray(out_ptr, dtype=np.int64)
    pair_ptr = d_pair if pair_ptr is None else np.ascontiguousarray(pair_ptr, dtype=np.int64)
    if not (grp_ptr.ndim == 1 and grp_ptr.shape[0] >= 1 and out_ptr.shape == grp_ptr.shape and pair_ptr.shape == grp_ptr.shape):
        raise ValueError("abx_dtw: grp_ptr, out_ptr and pair_ptr are (G + 1,) arrays")
    G, N = int(grp_ptr.shape[0]) - 1, int(tok_start.shape[0])
    if out is None:
        out = torch.empty(max(int(out_ptr[-1]), 0), dtype=torch.float32, device=feats.device)
    hb._want("abx_dtw", "out", out, torch.float32)
    dev = feats.device
    ptrs = torch.from_numpy(np.stack([grp_ptr, out_ptr, pair_ptr])).to(dev)  # (one upload)
    hb._call("fhvae_abx_dtw", hb._p(feats), feats.shape[0], feats.shape[1], hb._p(tok_start), hb._p(tok_len), N, int(max_len), hb._p(ptrs[0]),
             hb._p(ptrs[1]), hb._p(ptrs[2]), G, max(int(pair_ptr[-1]), 0), int(out.numel()), int(metric), hb._p(out), hb._p(status))
    return out


# ------------------------------------------------------------------------------------------------------------------- items
def read_items(path):
    """A ZeroSpeech / ABXpy .item file -> a list of (file, onset, offset, phone, prev, next, speaker), times in seconds, in file
    order.  The first line is the header (ITEM_HEADER; any line starting with '#' is taken as it); blank lines are skipped.  A
    line without seven fields, with a time that is no number, or with offset < onset raises ValueError naming its line."""
    items = []
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            s = line.strip()
            if not s or (no == 1 and s.startswith("#")):
                continue
            f = s.split()
            if len(f) != 7:
                raise ValueError("%s line %d: %d fields, not the 7 of '%s'" % (path, no, len(f), ITEM_HEADER))
            try:
                on, off = float(f[1]), float(f[2])
            except ValueError:
                raise ValueError("%s line %d: onset '%s' / offset '%s' are not numbers" % (path, no, f[1], f[2])) from None
            if not (np.isfinite(on) and np.isfinite(off) and off >= on):
                raise ValueError("%s line %d: onset %s and offset %s are not an interval" % (path, no, f[1], f[2]))
            items.append((f[0], on, off, f[3], f[4], f[5], f[6]))
    return items


def write_items(path, items):
    """The inverse of read_items."""
    with open(path, "w") as fh:
        fh.write(ITEM_HEADER + "\n")
        for it in items:
            fh.write("%s %.6f %.6f %s %s %s %s\n" % tuple(it))


def frame_range(onset, offset, n, frame_shift=0.010, frame_offset=0.0):
    """The frames f of an utterance of n frames with onset <= frame_offset + f frame_shift <= offset (to FRAME_EPS frames):
    (first, count), count 0 when there is none."""
    lo = int(np.ceil((onset - frame_offset) / frame_shift - FRAME_EPS))
    hi = int(np.floor((offset - frame_offset) / frame_shift + FRAME_EPS))
    lo, hi = max(lo, 0), min(hi, int(n) - 1)
    return lo, max(hi - lo + 1, 0)


def _ids(values):
    table, names, out = {}, [], np.empty(len(values), dtype=np.int64)
    for i, v in enumerate(values):
        if v not in table:
            table[v] = len(names)
            names.append(v)
        out[i] = table[v]
    return out, names


def tokens_from_items(items, keys, lengths, frame_shift=0.010, frame_offset=0.0, max_len=ABX_MAX_LEN, max_per_cell=20):
    """Item lines -> tokens on the frames of a corpus whose utterances `keys` have `lengths` frames and lie one after the other
    (frames.FramePool's layout).  A token is dropped, and counted under its reason, when its utterance is not in `keys`, when
    no frame falls into [onset, offset], or when more than max_len do; max_per_cell > 0 keeps the first max_per_cell tokens of
    every (phone, context, speaker) in file order (0: all).  Returns a dict of arrays, one entry per kept token:
      start  int64, the token's first frame in the corpus;  len  int32;  utt  the utterance's index in `keys`
      phone / ctx / spk  int64 ids into the lists "phones", "contexts" ((prev, next) pairs) and "speakers"
    and "dropped", the counts by DROP_REASONS."""
    if not frame_shift > 0:
        raise ValueError("frame_shift %g must be positive" % frame_shift)
    if max_len < 1 or max_len > ABX_MAX_LEN:
        raise ValueError("max_len %d must lie in [1, %d]" % (max_len, ABX_MAX_LEN))
    index = {k: i for i, k in enumerate(keys)}
    lengths = np.asarray(lengths, dtype=np.int64)
    base = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    dropped = dict.fromkeys(DROP_REASONS, 0)
    rows, cell_count = [], {}
    for name, on, off, phone, prev, nxt, spk in items:
        u = index.get(name)
        if u is None:
            dropped["unknown_utterance"] += 1
            continue
        first, count = frame_range(on, off, lengths[u], frame_shift, frame_offset)
        if count == 0:
            dropped["no_frames"] += 1
            continue
        if count > max_len:
            dropped["too_long"] += 1
            continue
        cell = (phone, prev, nxt, spk)
        seen = cell_count.get(cell, 0)
        if max_per_cell > 0 and seen >= max_per_cell:
            dropped["over_cell_cap"] += 1
            continue
        cell_count[cell] = seen + 1
        rows.append((u, first, count, phone, (prev, nxt), spk))
    phone, phones = _ids([r[3] for r in rows])
    ctx, contexts = _ids([r[4] for r in rows])
    spk, speakers = _ids([r[5] for r in rows])
    utt = np.asarray([r[0] for r in rows], dtype=np.int64)
    first = np.asarray([r[1] for r in rows], dtype=np.int64)
    return {"start": base[utt] + first if rows else np.zeros(0, np.int64), "len": np.asarray([r[2] for r in rows], dtype=np.int32),
            "utt": utt, "phone": phone, "ctx": ctx, "spk": spk, "phones": phones, "contexts": contexts, "speakers": speakers,
            "dropped": dropped}


# --------------------------------------------------------------------------------------------------------------- distances
def check_status(status):
    """Reads the status word (one host sync) and raises on what the kernels refused."""
    hip_ext.check_status("fhvae_abx_dtw", status, STATUS_BITS)


def pair_distances(feats_dev, tokens, metric="angular", max_block_elems=2 ** 26):
    """Yields (context id, idx, block) for every context of `tokens`: idx (n,) the positions in `tokens` of the context's tokens,
    in their order, and block (n, n) f32 numpy, block[a][b] the DTW distance between tokens idx[a] and idx[b] on the rows of
    feats_dev ((n_frames, D) f32 on the device).  One fhvae_abx_dtw call per chunk of contexts whose blocks together hold at
    most max_block_elems values; a single context above that raises ValueError naming it."""
    import torch

    code = METRICS[metric] if isinstance(metric, str) else int(metric)
    ctx = np.asarray(tokens["ctx"], dtype=np.int64)
    order = np.argsort(ctx, kind="stable")
    ids, counts = np.unique(ctx[order], return_counts=True)
    for c, n in zip(ids, counts):
        if int(n) * int(n) > max_block_elems:
            raise ValueError("context %s has %d tokens: its %d distances exceed max_block_elems = %d (lower max_per_cell)"
                             % (tokens["contexts"][int(c)], n, int(n) * int(n), max_block_elems))
    dev = feats_dev.device
    start = torch.from_numpy(np.asarray(tokens["start"], dtype=np.int64)[order]).to(dev)
    host_len = np.asarray(tokens["len"], dtype=np.int32)[order]
    length = torch.from_numpy(host_len).to(dev)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)  # (the groups' first tokens in `order`)
    status = hip_ext.status_word(dev)
    g0, G = 0, len(ids)
    while g0 < G:
        g1, elems = g0, 0
        while g1 < G and elems + int(counts[g1]) ** 2 <= max_block_elems:
            elems += int(counts[g1]) ** 2
            g1 += 1
        t0, t1 = int(first[g0]), int(first[g1])
        grp_ptr = first[g0:g1 + 1] - t0
        out_ptr, _ = group_ptrs(grp_ptr)
        out = dtw(feats_dev, start[t0:t1], length[t0:t1], grp_ptr, code, status, max_len=min(max(int(host_len[t0:t1].max()), 1), ABX_MAX_LEN))
        check_status(status)
        host = out.cpu().numpy()
        for g in range(g0, g1):
            n = int(counts[g])
            yield int(ids[g]), order[first[g]:first[g + 1]], host[out_ptr[g - g0]:out_ptr[g - g0 + 1]].reshape(n, n)
        g0 = g1


# ------------------------------------------------------------------------------------------------------------------ scores
def _counts(d_ax, d_bx, same):
    """d_ax (a, x), d_bx (b, x) -> for every B the number of (A, X) with d(A, X) > d(B, X) and with d(A, X) = d(B, X); `same`:
    A and X index the same tokens and A = X is no triple."""
    gt = d_ax[:, None, :] > d_bx[None, :, :]
    eq = d_ax[:, None, :] == d_bx[None, :, :]
    if same:
        k = np.arange(d_ax.shape[0])
        gt[k, :, k] = False
        eq[k, :, k] = False
    return gt.sum(axis=(0, 2), dtype=np.int64), eq.sum(axis=(0, 2), dtype=np.int64)


class _Task:
    """The cells of one task (within or across): per ordered (p, q) the sum of the cells' scores and their number."""

    def __init__(self, P):
        self.sum, self.cells = np.zeros((P, P)), np.zeros((P, P), dtype=np.int64)
        self.triples = self.gt = self.eq = 0

    def add(self, p, phone_b, gt, eq, per_b, P):
        """One X-side: B tokens of phones phone_b with their counts; every B stands in per_b triples."""
        n_b = np.bincount(phone_b, minlength=P)
        g, e = np.bincount(phone_b, weights=gt, minlength=P), np.bincount(phone_b, weights=eq, minlength=P)
        q = np.nonzero(n_b)[0]
        self.sum[p, q] += (g[q] + 0.5 * e[q]) / (n_b[q] * per_b)
        self.cells[p, q] += 1
        self.triples += int(n_b.sum()) * per_b
        self.gt += int(gt.sum())
        self.eq += int(eq.sum())

    def result(self):
        have = self.cells > 0
        by_pair = np.full(self.sum.shape, np.nan)
        by_pair[have] = self.sum[have] / self.cells[have]
        return (float(by_pair[have].mean()) if have.any() else float("nan")), by_pair


def abx_scores(blocks, tokens):
    """The ABX error of `tokens` from the blocks of pair_distances (any iterable of (context id, idx, block)).

    For a triple, err(A, B, X) = [d(A, X) > d(B, X)] + 1/2 [d(A, X) = d(B, X)].
      within   A, B, X share a context c and a speaker s; A and X have phone p, A != X; B has phone q != p.  The score of the cell
               (p, q, c, s) is the mean of err over its triples; then the mean over (c, s) for every ordered (p, q); then the mean
               over (p, q).
      across   the same with A and B of speaker s and X of a speaker s' != s; the cells are (p, q, c, s, s').
    A cell without a triple does not exist.  Computed per (context, speaker) sub-block with array comparisons, never triple by
    triple.  Returns {"within", "across" (nan without a cell), "cells_*", "triples_*", "gt_*", "eq_*" (the triples with
    d(A, X) > d(B, X) and with equality), "by_pair_*" ((phones, phones) arrays, nan where no cell), "tokens", "dropped"}."""
    phone, spk = np.asarray(tokens["phone"], dtype=np.int64), np.asarray(tokens["spk"], dtype=np.int64)
    P = len(tokens["phones"])
    within, across = _Task(P), _Task(P)
    for _, idx, block in blocks:
        idx = np.asarray(idx)
        ph, sp = phone[idx], spk[idx]
        speakers = np.unique(sp)
        for s in speakers:
            mine = np.nonzero(sp == s)[0]
            for p in np.unique(ph[mine]):
                a = mine[ph[mine] == p]
                b = mine[ph[mine] != p]
                if b.size == 0:
                    continue
                if a.size > 1:
                    gt, eq = _counts(block[np.ix_(a, a)], block[np.ix_(b, a)], True)
                    within.add(p, ph[b], gt, eq, a.size * (a.size - 1), P)
                for s2 in speakers:
                    x = np.nonzero((sp == s2) & (ph == p))[0]
                    if s2 == s or x.size == 0:
                        continue
                    gt, eq = _counts(block[np.ix_(a, x)], block[np.ix_(b, x)], False)
                    across.add(p, ph[b], gt, eq, a.size * x.size, P)
    res = {"tokens": int(phone.shape[0]), "dropped": dict(tokens.get("dropped", {}))}
    for name, task in (("within", within), ("across", across)):
        res[name], res["by_pair_" + name] = task.result()
        res["cells_" + name], res["triples_" + name] = int(task.cells.sum()), int(task.triples)
        res["gt_" + name], res["eq_" + name] = int(task.gt), int(task.eq)
    return res


def write_by_pair(path, res, phones):
    """One line per ordered (p, q) with a cell: p, q, the within and the across score ('nan' where that task has no cell)."""
    w, a = res["by_pair_within"], res["by_pair_across"]
    with open(path, "w") as fh:
        fh.write("phone\tother\twithin\tacross\n")
        for p in range(len(phones)):
            for q in range(len(phones)):
                if not (np.isnan(w[p, q]) and np.isnan(a[p, q])):
                    fh.write("%s\t%s\t%.6f\t%.6f\n" % (phones[p], phones[q], w[p, q], a[p, q]))


def evaluate(feats_dev, tokens, metric="angular", max_block_elems=2 ** 26):
    """pair_distances + abx_scores."""
    return abx_scores(pair_distances(feats_dev, tokens, metric, max_block_elems), tokens)
