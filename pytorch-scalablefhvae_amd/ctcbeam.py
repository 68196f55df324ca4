"""ctcbeam.py -- CTC prefix beam search with a phone bigram: the decoder that ctc.greedy is not.  greedy gives the
labelling of the single best path; the search sums a labelling's alignments, keeps the `beam` best prefixes per frame and can
add a language model on the labels.

  decode      the binding of include/fhvae_ctcbeam.h (csrc/ctcbeam.hip): every utterance's hypothesis and its score
  bigram      a label bigram with a start row and an end column from transcriptions, add-`smooth`, as log-probabilities
  table       the kernel's table: scale * bigram, a bonus on every label column
  search      the twin of ctc.greedy: the model's splice and logits, then decode
  tune        the (scale, bonus) of a grid with the lowest phone error rate on given utterances
  recognise   what ctc.recognise does with search in place of greedy

The definitions are this project's, written out in include/fhvae_ctcbeam.h and below.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import ctc
import hip_ext

#: include/fhvae_ctcbeam.h
CB_MAX_CLASSES = 128
CB_MAX_BEAM = 64
CB_NODE_BYTES = 16
CB_BAD_PTR, CB_EMPTY = 1, 2

_vp, _i64 = C.c_void_p, C.c_int64
#: the entry points of include/fhvae_ctcbeam.h: name -> (restype, argtypes).  Exported from libfhvae_hip.so but not part of
#: include/fhvae_hip.h (ABI 12 is unchanged), so they are bound from this table (hip_ext.load) and not in hip_binding.SIGNATURES
CB_SIGNATURES = {
    "fhvae_cb_ws_bytes": (_i64, [_i64, _i64]),
    "fhvae_cb_decode": (C.c_int, [_vp, _i64, _i64, _i64, _i64, _vp, _i64, _i64, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
}


def load_library():
    """hip_binding.load_library() with the entry points of include/fhvae_ctcbeam.h bound (argtypes from CB_SIGNATURES)."""
    return hip_ext.load(CB_SIGNATURES)


# ----------------------------------------------------------------------------------------------------------------- raw call
def decode(logits, utt_ptr, blank, beam=16, lm=None, class_beam=float("inf"), ws_limit=1 << 30, with_status=False):
    """fhvae_cb_decode.  logits (N, C) f32 on the device, utt_ptr (U + 1,) int64 (a device tensor or a host array), blank in
    [0, C), lm None or the (C + 1, C + 1) float64 table of table() (a host array, checked for NaN and +inf, or a device tensor) ->
        (tokens int32: the hypotheses one after the other, ptr int64 (U + 1,), score float64 (U,)), all on the device;
        with_status: and the OR of the utterances' status bits (CB_EMPTY)
    An utterance whose beam emptied out has no tokens and score -inf.  The rows are given a leading dimension that is a multiple
    of 4.  The utterances are split into consecutive groups whose trie nodes fit ws_limit bytes (one larger than the limit goes
    alone); an utterance's result is a function of its rows, the beam and the table alone, so the split changes no bit.  The
    status word and the lengths are read together at the end: the call's one wait for the kernels."""
    import torch

    import hip_binding as hb

    op, noun = "decode", "the CTC beam search"
    logits = hip_ext.device_tensor(op, "logits", logits, noun, torch.float32, 2)
    n_classes, blank, beam, class_beam = int(logits.shape[1]), int(blank), int(beam), float(class_beam)
    logits = hip_ext.class_rows(op, logits, noun, CB_MAX_CLASSES)
    if not 0 <= blank < n_classes:
        raise RuntimeError("%s: blank = %d lies outside the %d classes" % (op, blank, n_classes))
    if not 1 <= beam <= CB_MAX_BEAM:
        raise RuntimeError("%s: beam = %d, the kernel takes 1 to %d" % (op, beam, CB_MAX_BEAM))
    if not class_beam >= 0:
        raise RuntimeError("%s: class_beam = %r must not be negative" % (op, class_beam))
    dev = logits.device
    if lm is not None:
        on_device = isinstance(lm, torch.Tensor) and lm.is_cuda  # (a table on the device is taken as it is: reading it would wait)
        lm = lm if isinstance(lm, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(lm))
        if lm.dtype != torch.float64 or tuple(lm.shape) != (n_classes + 1, n_classes + 1):
            raise RuntimeError("%s: lm must be a (%d, %d) float64 table (got %s %s)" % (op, n_classes + 1, n_classes + 1, lm.dtype, tuple(lm.shape)))
        if not on_device and (bool(torch.isnan(lm).any()) or bool((lm == float("inf")).any())):
            raise RuntimeError("%s: lm holds NaN or +inf" % op)
        lm = lm.to(dev).contiguous()
    # a cell is the beam's trie nodes of one frame
    plan = hip_ext.BatchPlan(op, utt_ptr, None, dev, lambda utt, lab: np.diff(utt), beam * CB_NODE_BYTES, ws_limit)
    utt = plan.utt
    U, N = plan.U, int(logits.shape[0])
    if utt[-1] != N:
        raise RuntimeError("%s: utt_ptr ends at %d rows, logits holds %d" % (op, utt[-1], N))
    lib = load_library()
    hyp = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    out = torch.zeros(1 + U, dtype=torch.int32, device=dev)  # the status word, then the lengths: one copy reads both
    score = torch.empty(U, dtype=torch.float64, device=dev)
    if U == 0:
        res = (hyp[:0], torch.zeros(1, dtype=torch.int64, device=dev), score)
        return res + (0,) if with_status else res
    ws = torch.empty(max(int(lib.fhvae_cb_ws_bytes(plan.ws_cells, beam)), 256), dtype=torch.uint8, device=dev)
    no_rows = torch.zeros(1, (n_classes + 3) // 4 * 4, dtype=torch.float32, device=dev)  # (an empty array has no address)
    for a, b, ptrs in plan.parts:
        f0, f1 = int(utt[a]), int(utt[b])
        z = logits[f0:f1] if f1 > f0 else no_rows
        hb._call("fhvae_cb_decode", hb._p(z), z.stride(0), f1 - f0, n_classes, blank, hb._p(ptrs[0]), b - a, beam, class_beam,
                 hb._p(lm) if lm is not None else None, hb._p(hyp[f0:] if f1 > f0 else hyp), hb._p(out[1 + a:]), hb._p(score[a:b]),
                 hb._p(out), hb._p(ws), ws.numel())
    host = out.cpu().numpy()  # the one sync
    bits, lens = int(host[0]), host[1:].astype(np.int64)
    if bits & CB_BAD_PTR:
        raise RuntimeError("%s: the kernel refused the pointer array (nothing was written)" % op)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    take = np.repeat(utt[:-1] - ptr[:-1], lens) + np.arange(int(ptr[-1]), dtype=np.int64)  # where token k of the output lies in hyp
    res = (hyp[torch.from_numpy(take).to(dev)], torch.from_numpy(ptr).to(dev), score)
    return res + (bits & ~CB_BAD_PTR,) if with_status else res


# ----------------------------------------------------------------------------------------------------------- language model
def bigram(refs, n_classes, blank, smooth=1.0):
    """refs: one list of label ids per transcription (in [0, n_classes), none the blank) -> the (C + 1, C + 1) float64 table of
    log-probabilities log P(next | previous): row r the previous label, row C the sentence start; column c the next label,
    column C the sentence end.  P = (count + smooth) / (row total + smooth * C): a row is a distribution over the C - 1 labels
    and the end.  The blank's row and column are -inf; with smooth = 0 an unseen pair is -inf (forbidden) and a row without
    counts is -inf throughout."""
    n_classes, blank, smooth = int(n_classes), int(blank), float(smooth)
    if n_classes < 2 or not 0 <= blank < n_classes or not smooth >= 0:
        raise ValueError("bigram: %d classes, blank %d, smooth %r" % (n_classes, blank, smooth))
    counts = np.zeros((n_classes + 1, n_classes + 1))
    for ref in refs:
        prev = n_classes
        for v in ref:
            v = int(v)
            if not 0 <= v < n_classes or v == blank:
                raise ValueError("bigram: a transcription holds %d: no label of the %d classes (blank %d)" % (v, n_classes, blank))
            counts[prev, v] += 1.0
            prev = v
        counts[prev, n_classes] += 1.0
    counts[:, blank] = 0.0
    total = counts.sum(axis=1, keepdims=True) + smooth * n_classes
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(total > 0, np.log((counts + smooth) / np.where(total > 0, total, 1.0)), -np.inf)
    out[blank, :] = -np.inf
    out[:, blank] = -np.inf
    return out


def table(lm, scale, bonus):
    """bigram()'s table -> the kernel's: scale * lm (zeros at scale 0: no language model), then `bonus` added to every label
    column c < C (a reward per label put out, against the deletions a language model brings).  float64 numpy."""
    lm = np.asarray(lm, dtype=np.float64)
    if lm.ndim != 2 or lm.shape[0] != lm.shape[1] or lm.shape[0] < 3:
        raise ValueError("table: lm must be (C + 1, C + 1), got %s" % (lm.shape,))
    if not np.isfinite(scale) or not np.isfinite(bonus) or scale < 0:
        raise ValueError("table: scale = %r must be finite and not negative, bonus = %r finite" % (scale, bonus))
    out = np.zeros_like(lm) if scale == 0 else float(scale) * lm
    out[:, :-1] += float(bonus)
    return out


# ------------------------------------------------------------------------------------------------------------------- search
def _logits(op, x, utt_ptr, model, chunk=65536):
    """The model's logits on the rows of x spliced with its context, as ctc.greedy forms them: (N, ld) f32 rows, columns past C
    zero, and the pointer on the device."""
    import torch

    import probe

    w, b, mean, std, _ = probe._model_arrays(op, model)
    context = int(model["context"])
    x = hip_ext.device_tensor(op, "x", x, "the CTC beam search", torch.float32, 2)
    ptr = torch.as_tensor(utt_ptr, dtype=torch.int64).to(x.device)
    xs = ctc.splice(x, ptr, context)
    if xs.shape[1] != w.shape[1]:
        raise ValueError("%s: the spliced rows have %d columns, the model %d" % (op, xs.shape[1], w.shape[1]))
    tab, cst = probe.table(w, b, mean, std, device=x.device)
    n_classes = int(w.shape[0])
    return ctc.logits_of(xs.contiguous(), tab, cst, (n_classes + 3) // 4 * 4, chunk)[:, :n_classes], ptr


def _drop_blank(tokens, ptr, n_classes, blank):
    import phonerec

    ident = np.arange(n_classes, dtype=np.int32)
    ident[blank] = -1
    return phonerec.fold(tokens, ptr, ident)


def search(x, utt_ptr, model, beam=16, lm=None, scale=1.0, bonus=0.0, class_beam=float("inf"), chunk=65536):
    """x (N, D) f32 and utt_ptr (U + 1,) int64 on one device, a model of ctc.fit / ctc.load, lm None or bigram()'s table ->
    (tokens int32, ptr int64 (U + 1,)) as ctc.greedy, ready for phonerec.fold: the rows spliced with the model's context, the
    logits in row chunks, then decode with table(lm, scale, bonus)."""
    z, ptr = _logits("search", x, utt_ptr, model, chunk)
    blank = int(model["blank"])
    tab = table(lm, scale, bonus) if lm is not None else None
    tokens, hyp_ptr, _ = decode(z, ptr, blank, beam, tab, class_beam)
    return _drop_blank(tokens, hyp_ptr, int(z.shape[1]), blank)


def best_of(grid):
    """grid: [(scale, bonus, per)] -> the (scale, bonus) of the lowest per; a tie goes to the smaller scale, then the smaller bonus."""
    if not grid:
        raise ValueError("tune: the grid is empty")
    return min(grid, key=lambda g: (g[2], g[0], g[1]))[:2]


def tune(x, utt_ptr, refs, model, lm, beam=16, scales=(0.0, 0.5, 1.0, 1.5), bonuses=(0.0, 0.5, 1.0, 2.0), class_beam=float("inf"),
         phone_table=None):
    """The grid scales x bonuses on the utterances given (refs: one id list each): the logits are formed once, every point is one
    decode, its hypotheses and the refs go through phone_table (identity by default), phonerec.align and phonerec.error_rate.
    -> ((scale, bonus) of the lowest PER by best_of's rule, the grid [(scale, bonus, per)] in scale-major order)"""
    import phonerec

    z, ptr = _logits("tune", x, utt_ptr, model)
    n_classes, blank = int(z.shape[1]), int(model["blank"])
    fold = np.arange(n_classes, dtype=np.int32) if phone_table is None else np.asarray(phone_table, dtype=np.int32)
    ref_tok, ref_ptr = phonerec.fold(*phonerec.csr(refs, z.device), fold)
    grid = []
    for s in scales:
        for b in bonuses:
            tokens, hyp_ptr, _ = decode(z, ptr, blank, beam, table(lm, s, b), class_beam)
            hyp_tok, hp = phonerec.fold(*_drop_blank(tokens, hyp_ptr, n_classes, blank), fold)
            grid.append((float(s), float(b), float(phonerec.error_rate(phonerec.align(ref_tok, ref_ptr, hyp_tok, hp))["per"])))
    return best_of(grid), grid


def recognise(train_x, train_lengths, train_refs, test_x, test_lengths, test_refs, names, beam=16, scale=None, bonus=None,
              class_beam=float("inf"), smooth=1.0, scales=(0.0, 0.5, 1.0, 1.5), bonuses=(0.0, 0.5, 1.0, 2.0), l2=1e-4, iters=200,
              gtol=1e-5, context=0, init=None, phone_table=None, model=None):
    """ctc.recognise with search in place of greedy.  The model is fitted on the training transcriptions (or `model` is taken);
    the bigram is counted on the training transcriptions with add-`smooth`; (scale, bonus) is what is given, or with scale None
    tuned on the TRAINING utterances over scales x bonuses (no test utterance is seen).
    -> (model, report: error_rate's keys plus beam, lm_scale, bonus, class_beam (None: no class pruning), smooth, grid (None if not
    tuned); hyp, ref: the
    folded id lists per test utterance; lm: the bigram)"""
    import torch

    import phonerec

    n_phones = len(names)
    dev = test_x.device

    def ptr_of(lengths):
        return torch.from_numpy(np.concatenate([[0], np.cumsum(phonerec._host(lengths, np.int64))]).astype(np.int64)).to(dev)

    if model is None:
        model, _ = ctc.fit(train_x, ptr_of(train_lengths), train_refs, n_phones, l2=l2, iters=iters, gtol=gtol, context=context, init=init)
    fold = np.arange(n_phones, dtype=np.int32) if phone_table is None else np.asarray(phone_table, dtype=np.int32)
    if fold.shape != (n_phones,):
        raise ValueError("the phone table has %s entries for %d phones" % (fold.shape, n_phones))
    test_ptr = ptr_of(test_lengths)
    if int(test_ptr[-1]) != int(test_x.shape[0]) or len(test_refs) != int(test_ptr.shape[0]) - 1:
        raise ValueError("test_lengths and test_refs do not describe the %d test rows" % int(test_x.shape[0]))
    lm = bigram(train_refs, n_phones + 1, int(model["blank"]), smooth)
    grid = None
    if scale is None:
        (scale, bonus), grid = tune(train_x, ptr_of(train_lengths), train_refs, model, lm, beam, scales, bonuses, class_beam, fold)
    bonus = 0.0 if bonus is None else bonus
    hyp_tok, hyp_ptr = phonerec.fold(*search(test_x, test_ptr, model, beam, lm, scale, bonus, class_beam), fold)
    ref_tok, ref_ptr = phonerec.fold(*phonerec.csr(test_refs, dev), fold)
    report = phonerec.error_rate(phonerec.align(ref_tok, ref_ptr, hyp_tok, hyp_ptr))
    report.update({"beam": int(beam), "lm_scale": float(scale), "bonus": float(bonus), "class_beam": float(class_beam) if np.isfinite(class_beam) else None,
                   "smooth": float(smooth), "grid": grid})
    return model, report, phonerec.uncsr(hyp_tok, hyp_ptr), phonerec.uncsr(ref_tok, ref_ptr), lm
