"""segment.py -- unit sequences by segmentation: the cut of every utterance into segments of at most max_len frames,
and the codebook unit of every segment, that minimise the quantisation error plus a penalty `lam` per segment -- in place of
units.py's one arg-min per frame, which a single noisy frame splits.

  scores           the binding of fhvae_seg_scores (csrc/segment.hip): best unit and score of every (last frame, length) cell
  dp               the binding of fhvae_seg_dp: the optimal cut per utterance on those cells, per-frame unit and start flags
  segment          both over a corpus, in groups of utterances that fit a byte limit -> per-utterance (starts, units), costs
  to_items         segments as abx-layout item tuples (#phone "u<k>")
  boundary_scores  precision, recall, F, over-segmentation and R-value of hypothesis boundaries against an item file

The definitions (scores, ties, the recursion) are this project's, written out in include/fhvae_segment.h.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

import hip_ext

#: include/fhvae_segment.h
SEG_BAD_PTR, SEG_NOT_FINITE = 1, 2
SEG_MAX_LEN = 64
SEG_CHUNK_ROWS = 4096

_vp, _i64 = C.c_void_p, C.c_int64
#: the entry points of include/fhvae_segment.h: name -> (restype, argtypes).  Exported from libfhvae_hip.so but not part of
#: include/fhvae_hip.h (ABI 12 is unchanged), so they are bound from this table (hip_ext.load) and not in hip_binding.SIGNATURES
SEG_SIGNATURES = {
    "fhvae_seg_ws_bytes": (_i64, [_i64, _i64, _i64, _i64]),
    "fhvae_seg_scores": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "fhvae_seg_dp": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _i64, C.c_double, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
}

_STATUS = ((SEG_BAD_PTR, "utt_ptr is not monotone from 0 to the number of rows (nothing was written)"),
           (SEG_NOT_FINITE, "an utterance has no segmentation of finite cost (rows that are not finite?)"))


def load_library():
    """hip_binding.load_library() with the entry points of include/fhvae_segment.h bound (argtypes from SEG_SIGNATURES)."""
    return hip_ext.load(SEG_SIGNATURES)


def check_status(symbol, status):
    """Reads the status word (one host sync) and raises on what the kernels refused."""
    hip_ext.check_status(symbol, status, _STATUS)


def _max_len(op, max_len):
    max_len = int(max_len)
    if not 1 <= max_len <= SEG_MAX_LEN:
        raise ValueError("%s: max_len = %d must lie in [1, %d]" % (op, max_len, SEG_MAX_LEN))
    return max_len


# ---------------------------------------------------------------------------------------------------------------- raw calls
def scores(x, cent, utt_ptr, max_len, status=None, out=None):
    """fhvae_seg_scores.  x (N, D), cent (K, D) f32 rows as units.assign takes them, utt_ptr (U + 1,) int64, all on the device ->
    (score (N, max_len) f32, unit (N, max_len) int32): cell [n][l - 1] is the segment of l frames that ends at row n, +inf / -1
    where it would begin before its utterance.  With `status` (a hip_ext.status_word) the call only enqueues and the caller
    reads the word; without, it is read here (one host sync).  `out` gives the two arrays to write into."""
    import torch

    import hip_binding as hb
    import units

    op, noun = "seg_scores", "segmentation"
    lib = load_library()
    units._rows(op, "x", x)
    units._rows(op, "cent", cent, int(x.shape[1]))
    max_len = _max_len(op, max_len)
    utt_ptr = hip_ext.device_tensor(op, "utt_ptr", utt_ptr, noun, torch.int64, 1, contiguous=True)
    N, D, K, U = int(x.shape[0]), int(x.shape[1]), int(cent.shape[0]), int(utt_ptr.shape[0]) - 1
    if U < 1:
        raise RuntimeError("%s: utt_ptr must hold U + 1 >= 2 entries" % op)
    need = int(lib.fhvae_seg_ws_bytes(N, K, D, max_len))
    if need <= 0:
        raise ValueError("%s: %d rows / %d centroids lie outside the kernels' limits (%d rows, %d centroids)"
                         % (op, N, K, units.KM_MAX_ROWS, units.KM_MAX_CENT))
    ws = hip_ext.workspace("segment", x.device, need)
    if out is None:
        out = (torch.empty(N, max_len, dtype=torch.float32, device=x.device), torch.empty(N, max_len, dtype=torch.int32, device=x.device))
    score = hip_ext.device_tensor(op, "out[0]", out[0], noun, torch.float32, 2, (N, max_len), contiguous=True)
    unit = hip_ext.device_tensor(op, "out[1]", out[1], noun, torch.int32, 2, (N, max_len), contiguous=True)
    own = status is None
    status = hip_ext.status_word(x.device) if own else status
    hb._call("fhvae_seg_scores", hb._p(x), x.stride(0), N, D, hb._p(cent), cent.stride(0), K, max_len, hb._p(utt_ptr), U, hb._p(ws),
             ws.numel(), hb._p(score), hb._p(unit), hb._p(status))
    if own:
        check_status("fhvae_seg_scores", status)
    return score, unit


def dp(score, unit, utt_ptr, lam, status=None, out=None):
    """fhvae_seg_dp.  score, unit (N, max_len) of scores(), utt_ptr (U + 1,) int64 on the device, lam >= 0 ->
    (seg_unit (N,) int32, seg_start (N,) uint8, n_seg (U,) int32, cost (U,) float64).  The outputs have fixed shapes: nothing is
    read back to size them.  They are created as -1, 0, -1 and +inf, which is what an utterance without a finite cost keeps
    (SEG_NOT_FINITE); `out` gives the four arrays instead.  `status` as in scores()."""
    import torch

    import hip_binding as hb

    op, noun = "seg_dp", "segmentation"
    load_library()
    score = hip_ext.device_tensor(op, "score", score, noun, torch.float32, 2, contiguous=True)
    N, max_len = int(score.shape[0]), _max_len(op, score.shape[1])
    unit = hip_ext.device_tensor(op, "unit", unit, noun, torch.int32, 2, (N, max_len), contiguous=True)
    utt_ptr = hip_ext.device_tensor(op, "utt_ptr", utt_ptr, noun, torch.int64, 1, contiguous=True)
    U, lam = int(utt_ptr.shape[0]) - 1, float(lam)
    if U < 1:
        raise RuntimeError("%s: utt_ptr must hold U + 1 >= 2 entries" % op)
    if not lam >= 0.0:
        raise ValueError("%s: lam = %r must be at least 0" % (op, lam))
    dev = score.device
    if out is None:
        out = (torch.full((N,), -1, dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev),
               torch.full((U,), -1, dtype=torch.int32, device=dev), torch.full((U,), math.inf, dtype=torch.float64, device=dev))
    seg_unit = hip_ext.device_tensor(op, "out[0]", out[0], noun, torch.int32, 1, (N,), contiguous=True)
    seg_start = hip_ext.device_tensor(op, "out[1]", out[1], noun, torch.uint8, 1, (N,), contiguous=True)
    n_seg = hip_ext.device_tensor(op, "out[2]", out[2], noun, torch.int32, 1, (U,), contiguous=True)
    cost = hip_ext.device_tensor(op, "out[3]", out[3], noun, torch.float64, 1, (U,), contiguous=True)
    ws = hip_ext.workspace("segment", dev, max(N, 256))
    none = torch.zeros(4, dtype=torch.int32, device=dev)  # (an empty array has no address)
    own = status is None
    status = hip_ext.status_word(dev) if own else status
    hb._call("fhvae_seg_dp", hb._p(score if N else none), hb._p(unit if N else none), N, max_len, hb._p(utt_ptr), U, lam, hb._p(ws), ws.numel(),
             hb._p(seg_unit if N else none), hb._p(seg_start if N else none), hb._p(n_seg), hb._p(cost), hb._p(status))
    if own:
        check_status("fhvae_seg_dp", status)
    return seg_unit, seg_start, n_seg, cost


# ---------------------------------------------------------------------------------------------------------------- a corpus
def segment(x, cent, lengths, lam, max_len, ws_limit=1 << 30):
    """The utterances of `lengths` frames lie one after the other in x (N, D) f32 on the device; cent (K, D) ->
    (segs: per utterance (starts int64, units int32) numpy arrays, one entry per segment; costs (U,) float64 numpy).
    The utterances go through scores() and dp() in consecutive groups (hip_ext.groups) whose cells -- score and unit, 8 max_len
    bytes a frame -- and workspace stay under ws_limit bytes; an utterance's result is a function of its rows and the table
    alone, so the grouping changes no bit.  The status word is read once, at the end; an utterance without a finite cost
    raises RuntimeError."""
    import torch

    op = "segment"
    max_len = _max_len(op, max_len)
    lengths = np.asarray(lengths, dtype=np.int64)
    if lengths.ndim != 1 or (lengths < 0).any() or int(lengths.sum()) != int(x.shape[0]):
        raise ValueError("%s: %d rows for utterances of %d frames" % (op, int(x.shape[0]), int(lengths.sum())))
    U, dev = int(lengths.shape[0]), x.device
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    D, K = int(x.shape[1]), int(cent.shape[0])
    fixed = 4 * K + 256 + min(int(x.shape[0]), SEG_CHUNK_ROWS) * max_len * D * 4 + 512  # cn and a chunk of segment sums
    per_frame = 8 * max_len + 4 + 5 + 8  # cells, room, seg_unit and seg_start, the group's share of the pointers
    status = hip_ext.status_word(dev)
    starts_flag = np.zeros(int(ptr[-1]), dtype=np.uint8)
    frame_unit = np.zeros(int(ptr[-1]), dtype=np.int32)
    costs = np.zeros(U, dtype=np.float64)
    pending = []
    for a, b in hip_ext.groups(lengths * per_frame, max(int(ws_limit) - fixed, 1)):
        f0, f1 = int(ptr[a]), int(ptr[b])
        if f1 == f0:
            continue  # (empty utterances only: no segment, cost 0)
        p = torch.from_numpy(ptr[a:b + 1] - ptr[a]).to(dev)
        score, unit = scores(x[f0:f1], cent, p, max_len, status=status)
        seg_unit, seg_start, _, cost = dp(score, unit, p, lam, status=status)
        pending.append((a, b, f0, f1, seg_unit, seg_start, cost))
    check_status("fhvae_seg_dp", status)
    for a, b, f0, f1, seg_unit, seg_start, cost in pending:
        frame_unit[f0:f1], starts_flag[f0:f1], costs[a:b] = seg_unit.cpu().numpy(), seg_start.cpu().numpy(), cost.cpu().numpy()
    segs = []
    for u in range(U):
        a, b = int(ptr[u]), int(ptr[u + 1])
        st = np.nonzero(starts_flag[a:b])[0].astype(np.int64)
        segs.append((st, frame_unit[a:b][st].astype(np.int32)))
    return segs, costs


def frame_units(segs, lengths):
    """segs of segment() -> one int32 array per utterance with the segment's unit on every frame."""
    out = []
    for (st, un), T in zip(segs, lengths):
        out.append(np.repeat(np.asarray(un, dtype=np.int32), np.diff(np.concatenate([st, [int(T)]]))) if int(T) else np.zeros(0, np.int32))
    return out


# ------------------------------------------------------------------------------------------------------------------- items
def to_items(keys, speakers, segs, lengths, frame_shift=0.010, frame_offset=0.0):
    """Item tuples (abx.read_items' layout), one per segment: #phone "u<k>", onset = frame_offset + start * frame_shift, offset
    the same with the segment's last frame (so abx.frame_range gives back exactly its frames), the context columns the
    neighbouring segments' units of the utterance and `-` at its ends.  lengths: the frames per utterance (the last segment's
    end)."""
    if not len(keys) == len(speakers) == len(segs) == len(lengths):
        raise ValueError("to_items: %d keys, %d speakers, %d segmentations, %d lengths" % (len(keys), len(speakers), len(segs), len(lengths)))
    out = []
    for key, spk, (st, un), T in zip(keys, speakers, segs, lengths):
        ends = list(st[1:]) + [int(T)]
        names = ["u%d" % int(k) for k in un]
        for i, (a, b) in enumerate(zip(st, ends)):
            out.append((key, frame_offset + int(a) * frame_shift, frame_offset + (int(b) - 1) * frame_shift, names[i],
                        names[i - 1] if i > 0 else "-", names[i + 1] if i + 1 < len(names) else "-", spk))
    return out


def boundary_scores(hyp_starts, ref_items, keys, lengths, tol=0.020, frame_shift=0.010, frame_offset=0.0):
    """Hypothesis boundaries against the interior token onsets of an item list (abx.read_items' layout).
      hyp_starts   per utterance of `keys`, the first frame of every segment (segment()'s starts); the boundary in front of frame
                   f > 0 stands at frame_offset + (f - 0.5) * frame_shift (frame 0 and the utterance's end are no boundaries)
      reference    per utterance, the onsets of its tokens in time order but the first
    Matching is one-to-one and in time order within tol (to 1e-9 s): a two-pointer sweep, each reference boundary hit at most once.
    Utterances of `keys` without a token in ref_items are left out.  ->
      precision, recall, f, os = recall / precision - 1, r_value = 1 - (|r1| + |r2|) / 2 with r1 = sqrt((1 - recall)^2 + os^2) and
      r2 = (recall - 1 - os) / sqrt(2); hits, hyp_boundaries, ref_boundaries, utterances.  A figure is None without a boundary
      on the side it divides by."""
    if not len(hyp_starts) == len(keys) == len(lengths):
        raise ValueError("boundary_scores: %d segmentations, %d keys, %d lengths" % (len(hyp_starts), len(keys), len(lengths)))
    onsets = {}
    for it in ref_items:
        onsets.setdefault(it[0], []).append(float(it[1]))
    hits = nh = nr = utts = 0
    for key, st in zip(keys, hyp_starts):
        if key not in onsets:
            continue
        utts += 1
        ref = sorted(onsets[key])[1:]
        hyp = [frame_offset + (int(f) - 0.5) * frame_shift for f in st if int(f) > 0]
        nh, nr = nh + len(hyp), nr + len(ref)
        i = j = 0
        while i < len(hyp) and j < len(ref):
            if abs(hyp[i] - ref[j]) <= tol + 1e-9:
                hits, i, j = hits + 1, i + 1, j + 1
            elif hyp[i] < ref[j]:
                i += 1
            else:
                j += 1
    precision = hits / nh if nh else None
    recall = hits / nr if nr else None
    f = os_ = r_value = None
    if precision is not None and recall is not None:
        f = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
        if precision > 0:
            os_ = recall / precision - 1.0
            r1 = math.sqrt((1.0 - recall) ** 2 + os_ ** 2)
            r2 = (recall - 1.0 - os_) / math.sqrt(2.0)
            r_value = 1.0 - (abs(r1) + abs(r2)) / 2.0
    return {"precision": precision, "recall": recall, "f": f, "os": os_, "r_value": r_value, "hits": hits, "hyp_boundaries": nh,
            "ref_boundaries": nr, "utterances": utts}


# --------------------------------------------------------------------------------------------------------------- the corpus
def discover(rows, cent, keys, lengths, lam, max_len, k, items=None, frame_shift=0.010, frame_offset=0.0, tol=0.020,
             ws_limit=1 << 30):
    """What discover_units.py --segment and eval_model.py --units-segment add: rows (N, D) on the device as units.corpus_rows
    gives them, cent (K, width) numpy as units.discover returns it (zero-padded to D here) ->
    (block, segs, item tuples): block is the "segments" entry of units.json -- dur_penalty, max_seg_frames, segments,
    mean_frames, cost, bitrate_segments (units._bits over the segment-level sequences and the corpus duration) and, with `items`,
    boundary_scores' figures and units.unit_quality of the per-frame segment units (cluster_purity, phone_purity, pnmi,
    labelled_frames)."""
    import torch

    import units

    cent = np.asarray(cent, dtype=np.float32)
    table = torch.nn.functional.pad(torch.from_numpy(cent).to(rows.device), (0, int(rows.shape[1]) - cent.shape[1])).contiguous()
    segs, costs = segment(rows, table, lengths, lam, max_len, ws_limit)
    n = int(sum(len(st) for st, _ in segs))
    frames = int(np.sum(lengths))
    block = {"dur_penalty": float(lam), "max_seg_frames": int(max_len), "segments": n, "mean_frames": frames / n if n else 0.0,
             "cost": float(np.sum(costs, dtype=np.float64)),
             "bitrate_segments": units._bits([un for _, un in segs], frames * float(frame_shift))}
    speakers = ["-"] * len(keys)  # (the command lines know no speakers; abx.read_items takes the column as it is)
    if items is not None:
        block.update(boundary_scores([st for st, _ in segs], items, keys, lengths, tol, frame_shift, frame_offset))
        phones, names, _ = units.frame_phones(items, keys, lengths, frame_shift, frame_offset)
        per_frame = frame_units(segs, lengths)
        flat = np.concatenate(per_frame) if per_frame else np.zeros(0, np.int32)
        block.update(units.unit_quality(flat, phones, int(k), len(names)))
    return block, segs, to_items(keys, speakers, segs, lengths, frame_shift, frame_offset)
