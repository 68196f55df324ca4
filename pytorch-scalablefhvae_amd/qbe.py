"""qbe.py -- query-by-example search on frame-level representations ("Query by example"): where in a corpus does a
spoken example occur?  Every query (a term token of at most 64 frames) is aligned against every utterance by subsequence DTW, with
a free start and a free end in the utterance; the utterances are ranked by the cost of their best alignment.

  sdtw                the binding of include/fhvae_qbe.h (csrc/qbe.hip): the Q x U grid of one call
  queries_from_items  item lines (abx.read_items; the #phone column is the term) -> queries on the frames of a corpus
  truth_from_items    item lines -> the term tokens of the searched corpus, of any length (what rank_metrics scores against)
  search              the grid in chunks of queries, host arrays out
  rank_metrics        MAP, P@N, P@10 and the share of located tokens
  top_hits            the N best utterances per query

The definitions (frame cost, recursion, normalisation, ranking and scores) are this project's, written out in
include/fhvae_qbe.h and below; nothing here runs an external search tool.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import abx
import hip_ext

#: metric of fhvae_qbe_sdtw (abx.METRICS' codes), the bits of its int32 device status word and its limits (include/fhvae_qbe.h)
QBE_ANGULAR, QBE_COSINE = 0, 1
QBE_BAD_QUERY, QBE_BAD_PTR = 1, 2
QBE_MAX_DIM, QBE_MAX_QLEN = 128, 64
METRICS = {"angular": QBE_ANGULAR, "cosine": QBE_COSINE}

_vp, _i64 = C.c_void_p, C.c_int64
#: the entry point of include/fhvae_qbe.h: name -> (restype, argtypes).  Exported from libfhvae_hip.so but not part of
#: include/fhvae_hip.h (ABI 12 is unchanged), so it is bound from this table (hip_ext.load) and not in hip_binding.SIGNATURES
QBE_SIGNATURES = {
    "fhvae_qbe_sdtw": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _i64, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}

#: the messages of the status bits, in the order they are named (hip_ext.check_status)
STATUS_BITS = ((QBE_BAD_QUERY, "a query lies outside the features or is longer than its bound (at most %d frames)" % QBE_MAX_QLEN),
               (QBE_BAD_PTR, "utt_ptr is not monotone from 0 to the number of frames"))
DROP_REASONS = ("unknown_utterance", "no_frames", "too_long", "over_term_cap")


def load_library():
    """hip_binding.load_library() with the search entry point bound (argtypes from QBE_SIGNATURES)."""
    return hip_ext.load(QBE_SIGNATURES)


def sdtw(qfeats, q_start, q_len, feats, utt_ptr, metric, status, max_qlen=QBE_MAX_QLEN, profile=False, out=None):
    """fhvae_qbe_sdtw.  qfeats (nq_frames, D) and feats (n_frames, D) f32 (they may be one tensor), q_start (Q,) int64, q_len (Q,)
    int32, utt_ptr (U + 1,) int64 and status (1,) int32 on the device.  -> (best_cost (Q, U) f32, best_start, best_end (Q, U)
    int32, end_cost (Q, n_frames) f32, end_start (Q, n_frames) int32), the last two None unless profile.  A given `out` (the same
    five, None for a profile that is not wanted) is written into.  max_qlen: the caller's bound on q_len (a smaller one runs
    faster, the values are the same).  Only enqueues: read `status` afterwards."""
    import torch

    import hip_binding as hb

    load_library()
    hb._need_gpu(qfeats, feats, q_start, q_len, utt_ptr, status)
    hb._want("qbe_sdtw", "qfeats", qfeats, torch.float32, shape=(None, None))
    hb._want("qbe_sdtw", "feats", feats, torch.float32, shape=(None, qfeats.shape[1]))
    hb._want("qbe_sdtw", "q_start", q_start, torch.int64, ndim=1)
    hb._want("qbe_sdtw", "q_len", q_len, torch.int32, shape=tuple(q_start.shape))
    hb._want("qbe_sdtw", "utt_ptr", utt_ptr, torch.int64, ndim=1)
    hb._want("qbe_sdtw", "status", status, torch.int32, contiguous=False)
    if utt_ptr.shape[0] < 1:
        raise ValueError("qbe_sdtw: utt_ptr is a (U + 1,) tensor")
    Q, U, n_frames, dev = int(q_start.shape[0]), int(utt_ptr.shape[0]) - 1, int(feats.shape[0]), feats.device
    if out is None:
        out = (torch.empty(Q, U, dtype=torch.float32, device=dev), torch.empty(Q, U, dtype=torch.int32, device=dev),
               torch.empty(Q, U, dtype=torch.int32, device=dev),
               torch.empty(Q, n_frames, dtype=torch.float32, device=dev) if profile else None,
               torch.empty(Q, n_frames, dtype=torch.int32, device=dev) if profile else None)
    best_cost, best_start, best_end, end_cost, end_start = out
    hb._need_gpu(*out)
    hb._want("qbe_sdtw", "best_cost", best_cost, torch.float32, shape=(Q, U))
    hb._want("qbe_sdtw", "best_start", best_start, torch.int32, shape=(Q, U))
    hb._want("qbe_sdtw", "best_end", best_end, torch.int32, shape=(Q, U))
    hb._want("qbe_sdtw", "end_cost", end_cost, torch.float32, shape=(Q, n_frames), optional=True)
    hb._want("qbe_sdtw", "end_start", end_start, torch.int32, shape=(Q, n_frames), optional=True)
    hb._call("fhvae_qbe_sdtw", hb._p(qfeats), qfeats.shape[0], hb._p(feats), n_frames, feats.shape[1], hb._p(q_start), hb._p(q_len), Q,
             int(max_qlen), hb._p(utt_ptr), U, int(metric), hb._p(best_cost), hb._p(best_start), hb._p(best_end), hb._p(end_cost),
             hb._p(end_start), hb._p(status))
    return out


def check_status(status):
    """Reads the status word (one host sync) and raises on what the kernels refused."""
    hip_ext.check_status("fhvae_qbe_sdtw", status, STATUS_BITS)


# ------------------------------------------------------------------------------------------------------------------- items
def _corpus(keys, lengths):
    lengths = np.asarray(lengths, dtype=np.int64)
    return {k: i for i, k in enumerate(keys)}, lengths, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def queries_from_items(items, keys, lengths, frame_shift=0.010, frame_offset=0.0, max_len=QBE_MAX_QLEN, max_per_term=5):
    """Item lines -> queries on the frames of a corpus whose utterances `keys` have `lengths` frames and lie one after the other
    (frames.FramePool's layout).  The #phone column is the term.  A query is dropped, and counted under its reason, when its
    utterance is not in `keys`, when no frame falls into [onset, offset] (abx.frame_range), or when more than max_len do;
    max_per_term > 0 keeps the first max_per_term tokens of every term in file order (0: all).  Returns a dict of arrays, one
    entry per kept query:
      start  int64, the query's first frame in the corpus;  len  int32;  utt  the utterance's index in `keys`;  first  int64, the
      first frame inside that utterance;  term  int64 ids into the list "terms";  id  the strings `<term>_<k>`, k counting the
      term's kept tokens from 0
    and "dropped", the counts by DROP_REASONS."""
    if not frame_shift > 0:
        raise ValueError("frame_shift %g must be positive" % frame_shift)
    if max_len < 1 or max_len > QBE_MAX_QLEN:
        raise ValueError("max_len %d must lie in [1, %d]" % (max_len, QBE_MAX_QLEN))
    if max_per_term < 0:
        raise ValueError("max_per_term %d must not be negative" % max_per_term)
    index, lengths, base = _corpus(keys, lengths)
    dropped = dict.fromkeys(DROP_REASONS, 0)
    rows, seen = [], {}
    for name, on, off, term, _, _, _ in items:
        u = index.get(name)
        if u is None:
            dropped["unknown_utterance"] += 1
            continue
        first, count = abx.frame_range(on, off, lengths[u], frame_shift, frame_offset)
        if count == 0:
            dropped["no_frames"] += 1
            continue
        if count > max_len:
            dropped["too_long"] += 1
            continue
        k = seen.get(term, 0)
        if max_per_term > 0 and k >= max_per_term:
            dropped["over_term_cap"] += 1
            continue
        seen[term] = k + 1
        rows.append((u, first, count, term, "%s_%d" % (term, k)))
    term, terms = abx._ids([r[3] for r in rows])
    utt = np.asarray([r[0] for r in rows], dtype=np.int64)
    first = np.asarray([r[1] for r in rows], dtype=np.int64)
    return {"start": base[utt] + first if rows else np.zeros(0, np.int64), "len": np.asarray([r[2] for r in rows], dtype=np.int32),
            "utt": utt, "first": first, "term": term, "terms": terms, "id": [r[4] for r in rows], "dropped": dropped}


def truth_from_items(items, keys, lengths, frame_shift=0.010, frame_offset=0.0):
    """Item lines -> the term tokens of the searched corpus, of any length: {"utt" int64, "first", "last" int64 (frames inside
    the utterance, inclusive), "term" (the names, a list)}, one entry per token with a known utterance and at least one frame."""
    if not frame_shift > 0:
        raise ValueError("frame_shift %g must be positive" % frame_shift)
    index, lengths, _ = _corpus(keys, lengths)
    utt, first, last, term = [], [], [], []
    for name, on, off, t, _, _, _ in items:
        u = index.get(name)
        if u is None:
            continue
        f, count = abx.frame_range(on, off, lengths[u], frame_shift, frame_offset)
        if count > 0:
            utt.append(u), first.append(f), last.append(f + count - 1), term.append(t)
    return {"utt": np.asarray(utt, dtype=np.int64), "first": np.asarray(first, dtype=np.int64), "last": np.asarray(last, dtype=np.int64),
            "term": term}


# ------------------------------------------------------------------------------------------------------------------ search
def search(qfeats_dev, queries, feats_dev, utt_ptr, metric="angular", profile=False, max_cells=2 ** 26):
    """The Q x U grid of `queries` (queries_from_items' layout: "start" and "len" on the rows of qfeats_dev) against the
    utterances utt_ptr (U + 1,) (host integers) of feats_dev, both (frames, D) f32 on the device.  The queries are taken in
    order of length (a call's longest query picks the kernel instance, so a chunk also ends at 16 and at 32 frames) and cut
    into chunks whose outputs -- 3 U values per query, 2 n_frames more with `profile` -- stay under max_cells per call.  -> {"best_cost" (Q, U) f32, "best_start",
    "best_end" (Q, U) int32} as numpy in the queries' order, with profile also "end_cost" (Q, n_frames) f32 and "end_start"
    (Q, n_frames) int32."""
    import torch

    code = METRICS[metric] if isinstance(metric, str) else int(metric)
    utt_ptr = np.ascontiguousarray(utt_ptr, dtype=np.int64)
    U, n_frames, dev = len(utt_ptr) - 1, int(feats_dev.shape[0]), feats_dev.device
    host_start, host_len = np.asarray(queries["start"], dtype=np.int64), np.asarray(queries["len"], dtype=np.int32)
    Q = len(host_start)
    per_query = 3 * U + (2 * n_frames if profile else 0)
    step = max(1, max_cells // max(per_query, 1))
    res = {"best_cost": np.full((Q, U), np.inf, dtype=np.float32), "best_start": np.full((Q, U), -1, dtype=np.int32),
           "best_end": np.full((Q, U), -1, dtype=np.int32)}
    if profile:
        res["end_cost"], res["end_start"] = np.zeros((Q, n_frames), dtype=np.float32), np.zeros((Q, n_frames), dtype=np.int32)
    if Q == 0 or U == 0:
        return res
    order = np.argsort(host_len, kind="stable")
    start, length = torch.from_numpy(host_start[order]).to(dev), torch.from_numpy(host_len[order]).to(dev)
    ptr = torch.from_numpy(utt_ptr).to(dev)
    status = hip_ext.status_word(dev)
    names = ("best_cost", "best_start", "best_end", "end_cost", "end_start")
    sorted_len = host_len[order]
    a = 0
    while a < Q:
        # (a chunk ends where the next kernel instance begins: queries of up to 16, up to 32 and up to 64 frames)
        b = min(a + step, Q, int(np.searchsorted(sorted_len, 16 if sorted_len[a] <= 16 else (32 if sorted_len[a] <= 32 else QBE_MAX_QLEN), "right")))
        b = max(b, a + 1)  # (a query the kernel will refuse still gets its call)
        bound = min(max(int(sorted_len[b - 1]), 1), QBE_MAX_QLEN)
        out = sdtw(qfeats_dev, start[a:b], length[a:b], feats_dev, ptr, code, status, max_qlen=bound, profile=profile)
        check_status(status)
        for name, t in zip(names, out):
            if t is not None:
                res[name][order[a:b]] = t.cpu().numpy()
        a = b
    return res


# ------------------------------------------------------------------------------------------------------------------ scores
def rank_metrics(best_cost, best_start, best_end, queries, truth, same_corpus=True):
    """How well the grid of `search` finds the term tokens `truth` (truth_from_items, on the searched corpus), in float64.

    Per query: with same_corpus (the queries were cut from the searched corpus) the query's own utterance is no candidate.
    A candidate is relevant when it holds a truth token of the query's term; a query without a relevant candidate is dropped
    and counted ("no_target").  The candidates are ranked by best_cost ascending, equal costs by utterance index.
      map      the mean over the queries of the average precision: the mean, over the relevant utterances, of (relevant
               utterances at or above its rank) / (its rank)
      p_at_n   the mean of (relevant among the first N) / N, N the query's number of relevant utterances
      p_at_10  the mean of (relevant among the first K) / K, K = min(10, candidates)
      located  over all (query, relevant utterance) pairs, the share whose detection [best_start, best_end] overlaps a truth
               token [first, last] of the term in that utterance by at least half of the shorter of the two (in frames)
    -> {"map", "p_at_n", "p_at_10", "located" (None without a scored query), "queries" (scored), "no_target"}."""
    cost = np.asarray(best_cost, dtype=np.float64)
    bs, be = np.asarray(best_start, dtype=np.int64), np.asarray(best_end, dtype=np.int64)
    Q, U = cost.shape
    by_term = {}
    for k, t in enumerate(truth["term"]):
        by_term.setdefault(t, []).append(k)
    t_utt, t_first, t_last = (np.asarray(truth[k], dtype=np.int64) for k in ("utt", "first", "last"))
    ap, pn, p10, found, pairs, no_target = [], [], [], 0, 0, 0
    for q in range(Q):
        tok = np.asarray(by_term.get(queries["terms"][int(queries["term"][q])], []), dtype=np.int64)
        cand = np.ones(U, dtype=bool)
        if same_corpus:
            cand[int(queries["utt"][q])] = False
        rel = np.zeros(U, dtype=bool)
        rel[t_utt[tok]] = True
        rel &= cand
        n_rel = int(rel.sum())
        if n_rel == 0:
            no_target += 1
            continue
        idx = np.nonzero(cand)[0]
        ranked = idx[np.lexsort((idx, cost[q, idx]))]  # (by cost, then by utterance index)
        hit = rel[ranked]
        at = np.nonzero(hit)[0]
        ap.append(float(np.mean(np.arange(1, n_rel + 1, dtype=np.float64) / (at + 1.0))))
        pn.append(float(hit[:n_rel].sum()) / n_rel)
        K = min(10, len(ranked))
        p10.append(float(hit[:K].sum()) / K)
        for u in np.nonzero(rel)[0]:
            d0, d1 = bs[q, u], be[q, u]
            mine = tok[t_utt[tok] == u]
            over = np.minimum(d1, t_last[mine]) - np.maximum(d0, t_first[mine]) + 1
            shorter = np.minimum(d1 - d0 + 1, t_last[mine] - t_first[mine] + 1)
            found += int(d1 >= 0 and np.any(2 * over >= shorter))
            pairs += 1
    mean = lambda v: float(np.mean(np.asarray(v, dtype=np.float64))) if v else None
    return {"map": mean(ap), "p_at_n": mean(pn), "p_at_10": mean(p10), "located": found / pairs if pairs else None,
            "queries": len(ap), "no_target": no_target}


def top_hits(best_cost, best_start, best_end, queries, top, same_corpus=True):
    """-> per query the list of (rank from 1, utterance index, start frame, end frame, cost) of its `top` best candidates, in
    rank_metrics' order; an utterance without a detection (empty) is no hit."""
    cost = np.asarray(best_cost, dtype=np.float64)
    Q, U = cost.shape
    hits = []
    for q in range(Q):
        idx = np.arange(U)
        if same_corpus:
            idx = idx[idx != int(queries["utt"][q])]
        ranked = idx[np.lexsort((idx, cost[q, idx]))][:top]
        hits.append([(r + 1, int(u), int(best_start[q][u]), int(best_end[q][u]), float(cost[q, u])) for r, u in enumerate(ranked)
                     if best_end[q][u] >= 0])
    return hits


def write_hits(path, hits, queries, keys, frame_shift=0.010, frame_offset=0.0):
    """hits.tsv: query id, term, rank, utterance key, start s, end s (the times of the detection's first and last frame), cost."""
    with open(path, "w") as fh:
        fh.write("query\tterm\trank\tutterance\tstart\tend\tcost\n")
        for q, rows in enumerate(hits):
            term = queries["terms"][int(queries["term"][q])]
            for rank, u, s, e, c in rows:
                fh.write("%s\t%s\t%d\t%s\t%.3f\t%.3f\t%.6f\n" % (queries["id"][q], term, rank, keys[u], frame_offset + s * frame_shift,
                                                              frame_offset + e * frame_shift, c))


def evaluate(qfeats_dev, queries, feats_dev, utt_ptr, truth, metric="angular", same_corpus=True, max_cells=2 ** 26):
    """search + rank_metrics -> (the metrics, the grid)."""
    grid = search(qfeats_dev, queries, feats_dev, utt_ptr, metric, max_cells=max_cells)
    return rank_metrics(grid["best_cost"], grid["best_start"], grid["best_end"], queries, truth, same_corpus), grid


def corpus_rows(model, pool, on, batch_size=16384):
    """The (total frames, D) rows of a shift-1 frames.FramePool that are searched: "z1", frames.encode_frames' frame-level z1;
    "feats", the normalised input.  More than QBE_MAX_DIM values per frame raise ValueError."""
    import frames

    return checked_rows(frames.corpus_rows(model, pool, on, "search", batch_size), on)


def checked_rows(rows, on):
    if rows.shape[1] > QBE_MAX_DIM:
        raise ValueError("%s has %d values per frame, the DTW kernel takes at most %d" % (on, rows.shape[1], QBE_MAX_DIM))
    return rows.contiguous()


def utt_ptr_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)
