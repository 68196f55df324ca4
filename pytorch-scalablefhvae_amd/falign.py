"""falign.py -- forced alignment of transcriptions to frame-level scores: a model trained from the token order
alone (ctc.py), or a frame probe (probe.py), and a transcription give back TIMES, as an item file the rest of the chain reads.

  align            the binding of include/fhvae_falign.h (csrc/falign.hip): every utterance's best path through the trellis of
                   its transcription, the first and last frame of every token and the path's score
  scores_of        the logits of a ctc.fit model (spliced by its context) or of a probe model
  spans            (first, last) frame per token from the kernel's seg, under the "own" or the "follow" rule
  items            item tuples for abx.write_items from the spans
  read_text        Kaldi's `text` format: `key tok tok ...`
  boundary_report  onsets and frame agreement of an aligned item list against a reference one
  path_logprob     the best path's log-probability under the row-wise softmax (torch float64; not pinned by a test)

Two topologies (the header has the definition): CTC (blank >= 0: 2 L + 1 states, the blank between the labels) and HMM
(blank == -1: one state per label, stay or move on).  The definitions are this project's.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import ctc
import hip_ext

#: include/fhvae_falign.h
FA_MAX_CLASSES = 128
FA_MAX_LABELS = 256
FA_BAD_PTR, FA_BAD_LABEL, FA_INFEASIBLE = 1, 2, 4

_vp, _i64 = C.c_void_p, C.c_int64
#: the entry points of include/fhvae_falign.h: name -> (restype, argtypes).  Exported from libfhvae_hip.so but not part of
#: include/fhvae_hip.h (ABI 12 is unchanged), so they are bound from this table (hip_ext.load) and not in hip_binding.SIGNATURES
FA_SIGNATURES = {
    "fhvae_fa_ws_bytes": (_i64, [_i64]),
    "fhvae_fa_align": (C.c_int, [_vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
}


def load_library():
    """hip_binding.load_library() with the entry points of include/fhvae_falign.h bound (argtypes from FA_SIGNATURES)."""
    return hip_ext.load(FA_SIGNATURES)


# ----------------------------------------------------------------------------------------------------------------- raw call
def cells(utt_ptr, lab_ptr, blank):
    """The back-pointer bytes every utterance needs: T_u S_u with S_u = 2 L_u + 1 (blank >= 0) or L_u (blank == -1); an utterance
    the kernel refuses (L_u above 256) needs none."""
    T, L = np.diff(np.asarray(utt_ptr, dtype=np.int64)), np.diff(np.asarray(lab_ptr, dtype=np.int64))
    return np.where(L > FA_MAX_LABELS, 0, T * (2 * L + 1 if int(blank) >= 0 else L))


def align(scores, utt_ptr, labels, lab_ptr, blank, ws_limit=1 << 30):
    """fhvae_fa_align.  scores (N, C) f32, utt_ptr (U + 1,) int64, labels int32, lab_ptr (U + 1,) int64, all on the device; blank
    in [0, C) (CTC topology) or -1 (HMM topology) ->
        (state (N,) int32, seg (n_labels, 2) int32: first and last frame of every label within its utterance,
         score (U,) float64: the best path's sum of raw scores, bits: the OR of FA_BAD_LABEL and FA_INFEASIBLE over the utterances)
    An utterance without a path has score -inf and -1 in state and seg.  The rows are given a leading dimension that is a multiple
    of 4.  The utterances are split into consecutive groups whose back-pointers fit ws_limit bytes (one larger than the limit goes
    alone); an utterance's result is a function of its rows and labels alone, so the split changes no bit.  The pointers are
    copied to the host to plan the groups and the status word is read once, at the end: the call's one wait for the kernels."""
    import torch

    import hip_binding as hb

    op = "align"
    noun = "forced alignment"
    scores = hip_ext.device_tensor(op, "scores", scores, noun, torch.float32, 2)
    hip_ext.device_tensor(op, "utt_ptr", utt_ptr, noun, torch.int64, 1)
    labels = hip_ext.device_tensor(op, "labels", labels, noun, torch.int32, 1).contiguous()
    hip_ext.device_tensor(op, "lab_ptr", lab_ptr, noun, torch.int64, 1)
    n_classes, blank = int(scores.shape[1]), int(blank)
    scores = hip_ext.class_rows(op, scores, noun, FA_MAX_CLASSES)
    if not -1 <= blank < n_classes:
        raise RuntimeError("%s: blank = %d is neither a class of the %d nor -1" % (op, blank, n_classes))
    dev = scores.device
    plan = hip_ext.BatchPlan(op, utt_ptr, lab_ptr, dev, lambda utt, lab: cells(utt, lab, blank), 1, ws_limit)  # (a cell is a byte)
    utt, lab = plan.utt, plan.lab
    U, N, n_labels = plan.U, int(scores.shape[0]), int(lab[-1])
    if utt[-1] != N or n_labels > labels.shape[0]:
        raise RuntimeError("%s: the pointers end at %d rows and %d labels, the arrays hold %d and %d" % (op, utt[-1], n_labels, N, labels.shape[0]))
    lib = load_library()
    state = torch.empty(N, dtype=torch.int32, device=dev)
    seg = torch.empty(n_labels, 2, dtype=torch.int32, device=dev)
    score = torch.empty(U, dtype=torch.float64, device=dev)
    if U == 0:
        return state, seg, score, 0
    ws = torch.empty(max(int(lib.fhvae_fa_ws_bytes(plan.ws_cells)), 256), dtype=torch.uint8, device=dev)
    status = hip_ext.status_word(dev)
    no_rows = torch.zeros(1, (n_classes + 3) // 4 * 4, dtype=torch.float32, device=dev)  # (an empty array has no address)
    no_int = torch.zeros(2, dtype=torch.int32, device=dev)
    for a, b, ptrs in plan.parts:
        f0, f1, l0, l1 = int(utt[a]), int(utt[b]), int(lab[a]), int(lab[b])
        z = scores[f0:f1] if f1 > f0 else no_rows
        hb._call("fhvae_fa_align", hb._p(z), z.stride(0), f1 - f0, n_classes, blank, hb._p(ptrs[0]), hb._p(labels[l0:l1] if l1 > l0 else no_int),
                 hb._p(ptrs[1]), hb._p(ptrs[2]), b - a, hb._p(state[f0:f1] if f1 > f0 else no_int), hb._p(seg[l0:l1] if l1 > l0 else no_int),
                 hb._p(score[a:b]), hb._p(status), hb._p(ws), ws.numel())
    bits = int(status.item())
    if bits & FA_BAD_PTR:
        raise RuntimeError("%s: the kernel refused the pointer arrays (nothing was written)" % op)
    return state, seg, score, bits


def scores_of(x, utt_ptr, model, chunk=65536):
    """x (N, D) f32 and utt_ptr (U + 1,) on one device, a model of ctc.fit / ctc.load (it has "context": the rows are spliced by
    it) or a probe model -> (N, C) f32 logits x' @ tab.T + cst with probe.table's (tab, cst): ctc.splice, ctc.logits_of."""
    import torch

    import probe

    w, b, mean, std, _ = probe._model_arrays("scores_of", model)
    context = int(model["context"]) if "context" in model else 0
    x = hip_ext.device_tensor("scores_of", "x", x, "forced alignment", torch.float32, 2)
    xs = ctc.splice(x, torch.as_tensor(utt_ptr, dtype=torch.int64).to(x.device), context)
    if xs.shape[1] != w.shape[1]:
        raise ValueError("scores_of: the rows have %d columns (context %d), the model %d" % (xs.shape[1], context, w.shape[1]))
    tab, cst = probe.table(w, b, mean, std, device=x.device)
    return ctc.logits_of(xs.contiguous(), tab, cst, int(w.shape[0]), chunk)


def path_logprob(scores, utt_ptr, score):
    """score - sum_t logsumexp(z_t) per utterance: the log-probability of the best path under the row-wise softmax, with torch
    float64 ops (-inf stays -inf).  A convenience for reports: its sums are torch's, no test pins their bits."""
    import torch

    ptr = torch.as_tensor(utt_ptr, dtype=torch.int64).to(scores.device)
    lse = torch.logsumexp(scores.double(), dim=1)
    run = torch.cat([lse.new_zeros(1), torch.cumsum(lse, dim=0)])
    return score - (run[ptr[1:]] - run[ptr[:-1]])


# -------------------------------------------------------------------------------------------------------------------- spans
RULES = ("own", "follow")


def spans(seg, lab_ptr, lengths, rule="follow"):
    """seg (n_labels, 2) of align(), lab_ptr (U + 1,), lengths (U,) frames per utterance -> (n_labels, 2) int64 numpy: the first
    and the last frame of every token, -1 for the tokens of an utterance that was not aligned.
      "own"     the frames the path sits in the label's own state
      "follow"  the CTC default: a token runs to the frame before the next token's first, and the last token to T - 1 (the blanks
                after a label belong to it; leading blanks belong to no token)
    In HMM topology every frame is some label's own, so both rules agree (and nothing trails)."""
    if rule not in RULES:
        raise ValueError("spans: rule %r is none of %s" % (rule, RULES))
    seg = np.asarray(seg.cpu() if hasattr(seg, "cpu") else seg).astype(np.int64).reshape(-1, 2)
    lab = np.asarray(lab_ptr.cpu() if hasattr(lab_ptr, "cpu") else lab_ptr).astype(np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    if lab.shape[0] != lengths.shape[0] + 1 or lab[-1] != seg.shape[0]:
        raise ValueError("spans: lab_ptr, lengths and seg describe %d, %d and %d" % (lab.shape[0] - 1, lengths.shape[0], seg.shape[0]))
    out = seg.copy()
    if rule == "follow":
        for u in range(lengths.shape[0]):
            a, b = int(lab[u]), int(lab[u + 1])
            if b > a and seg[a, 0] >= 0:
                out[a:b - 1, 1] = seg[a + 1:b, 0] - 1
                out[b - 1, 1] = lengths[u] - 1
    return out


def items(keys, speakers, spans, refs, names, frame_shift=0.010, frame_offset=0.0):
    """Item tuples (abx.read_items' layout) of the aligned tokens: keys and speakers per utterance, spans (n_labels, 2) of spans(),
    refs one list of ids into `names` per utterance.  onset = frame_offset + first * frame_shift, offset the same with last, so
    abx.frame_range gives back exactly (first, last - first + 1).  The context columns hold the neighbouring tokens of the
    utterance, `-` where there is none (as tools/timit_items.py --tier phn-all).  An utterance that was not aligned (-1) gives no
    item."""
    if sum(len(r) for r in refs) != len(spans) or not len(keys) == len(speakers) == len(refs):
        raise ValueError("items: the %d transcriptions hold %d tokens, spans %d" % (len(refs), sum(len(r) for r in refs), len(spans)))
    out, k = [], 0
    for key, spk, ref in zip(keys, speakers, refs):
        for i, tok in enumerate(ref):
            first, last = int(spans[k][0]), int(spans[k][1])
            k += 1
            if first < 0:
                continue
            out.append((key, frame_offset + first * frame_shift, frame_offset + last * frame_shift, names[tok],
                        names[ref[i - 1]] if i > 0 else "-", names[ref[i + 1]] if i + 1 < len(ref) else "-", spk))
    return out


def read_text(path):
    """Kaldi's `text`: one `key tok tok ...` line per utterance -> (keys, token lists) in file order.  A line with a key only is
    an empty transcription; blank lines are skipped; a key met twice raises ValueError naming its line."""
    keys, toks, seen = [], [], {}
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            f = line.split()
            if not f:
                continue
            if f[0] in seen:
                raise ValueError("%s line %d: key '%s' was given on line %d already" % (path, no, f[0], seen[f[0]]))
            seen[f[0]] = no
            keys.append(f[0])
            toks.append(f[1:])
    return keys, toks


def _by_utterance(item_list):
    per = {}
    for no, it in enumerate(item_list):
        per.setdefault(it[0], []).append((it[1], no, it))
    return {k: [it for _, _, it in sorted(v)] for k, v in per.items()}


def boundary_report(hyp_items, ref_items, frame_shift=0.010):
    """Aligned items against reference items (both abx.read_items' layout), over the utterances both hold and whose token
    sequences (in onset order) agree ->
      utterances, tokens       what was compared
      skipped_sequence         utterances of both whose token sequences differ (they are not compared)
      onset_mae                the mean absolute onset deviation in seconds
      within_10ms, within_20ms the shares of onsets at most that far from the reference (to 1e-9 s)
      frame_agreement          the share of the reference tokens' frames (frames of `frame_shift` from the utterance's first
                               reference onset) that lie in the same token of the hypothesis
    Without a compared token the figures are None."""
    hyp, ref = _by_utterance(hyp_items), _by_utterance(ref_items)
    dev, agree, total, utts, skipped = [], 0, 0, 0, 0
    for key in ref:
        if key not in hyp:
            continue
        h, r = hyp[key], ref[key]
        if [it[3] for it in h] != [it[3] for it in r]:
            skipped += 1
            continue
        utts += 1
        for a, b in zip(h, r):
            dev.append(abs(a[1] - b[1]))
            lo, hi = int(round(b[1] / frame_shift)), int(round(b[2] / frame_shift))
            ha, hb_ = int(round(a[1] / frame_shift)), int(round(a[2] / frame_shift))
            total += hi - lo + 1
            agree += max(min(hi, hb_) - max(lo, ha) + 1, 0)
    dev = np.asarray(dev, dtype=np.float64)
    return {"utterances": utts, "tokens": int(dev.shape[0]), "skipped_sequence": skipped,
            "onset_mae": float(dev.mean()) if dev.size else None,
            "within_10ms": float(np.mean(dev <= 0.010 + 1e-9)) if dev.size else None,
            "within_20ms": float(np.mean(dev <= 0.020 + 1e-9)) if dev.size else None,
            "frame_agreement": float(agree) / total if total else None}
