"""phonerec.py -- phone recognition on frame-level representations: the frame probe's per-frame scores become a
phone sequence by a Viterbi pass under a frame-level phone bigram, and the sequence is scored against the transcription by the
phone error rate (PER), the number the FHVAE papers print.

  viterbi, align   the bindings of include/fhvae_viterbi.h (csrc/viterbi.hip): the best state sequence of every utterance; the
                   substitutions, deletions, insertions and correct tokens of every (reference, hypothesis) pair
  transitions      the frame-level bigram (log transition table and log initial scores) counted on labelled frames
  emissions        scaled log-likelihoods of a probe model: acoustic_scale (log softmax - prior_scale log prior)
  collapse, fold   runs of equal states merged per utterance; ids mapped through a table that may delete (the 61 -> 39 fold)
  read_phone_map, references, error_rate, recognise

The definitions are this project's, written out in include/fhvae_viterbi.h and below; nothing here runs Kaldi, HTK or sclite.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import hip_ext

#: include/fhvae_viterbi.h
VIT_MAX_STATES = 128
EDIT_MAX_REF = 256
VIT_BAD_PTR = 1
EDIT_BAD_PTR, EDIT_BAD_REF = 1, 2

_vp, _i64 = C.c_void_p, C.c_int64
#: the entry points of include/fhvae_viterbi.h: name -> (restype, argtypes).  Exported from libfhvae_hip.so but not part of
#: include/fhvae_hip.h (ABI 12 is unchanged), so they are bound from this table (hip_ext.load) and not in hip_binding.SIGNATURES
PHONEREC_SIGNATURES = {
    "fhvae_vit_ws_bytes": (_i64, [_i64, _i64]),
    "fhvae_vit_decode": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
    "fhvae_edit_align": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
}


def load_library():
    """hip_binding.load_library() with the entry points of include/fhvae_viterbi.h bound (argtypes from PHONEREC_SIGNATURES)."""
    return hip_ext.load(PHONEREC_SIGNATURES)


# ---------------------------------------------------------------------------------------------------------------- raw calls
def _device(op, name, t, dtype, dim):
    return hip_ext.device_tensor(op, name, t, "phone recognition", dtype, dim)


def _ptr(op, name, t):
    import torch

    t = _device(op, name, t, torch.int64, 1)
    if t.shape[0] < 1:
        raise RuntimeError("%s: %s must hold U + 1 entries" % (op, name))
    return t.contiguous()


def viterbi(emit, utt_ptr, trans, init, fin=None):
    """fhvae_vit_decode.  emit (N, C) f32, utt_ptr (U + 1,) int64, trans (C, C) f32, init (C,) f32, fin (C,) f32 or None, all on
    the device -> (path (N,) int32, score (U,) f32).  The rows are given a leading dimension that is a multiple of 4; the
    back-pointer workspace (one byte per frame and state) lives for the call.  One host sync, for the status word."""
    import torch

    import hip_binding as hb

    op = "viterbi"
    emit = _device(op, "emit", emit, torch.float32, 2)
    utt_ptr = _ptr(op, "utt_ptr", utt_ptr)
    trans = _device(op, "trans", trans, torch.float32, 2).contiguous()
    init = _device(op, "init", init, torch.float32, 1).contiguous()
    if fin is not None:
        fin = _device(op, "fin", fin, torch.float32, 1).contiguous()
    N, n_states = int(emit.shape[0]), int(emit.shape[1])
    if n_states < 1 or n_states > VIT_MAX_STATES:
        raise RuntimeError("%s: %d states, the decoder takes 1 to %d" % (op, n_states, VIT_MAX_STATES))
    if tuple(trans.shape) != (n_states, n_states) or tuple(init.shape) != (n_states,) or (fin is not None and tuple(fin.shape) != (n_states,)):
        raise RuntimeError("%s: trans, init and fin must be (%d, %d), (%d,), (%d,)" % (op, n_states, n_states, n_states, n_states))
    lib = load_library()
    dev = emit.device
    if N == 0:
        emit = torch.zeros(1, 4, dtype=torch.float32, device=dev)
    elif not hip_ext.rows_dense(emit, n_states):  # (else: taken as it is)
        emit = torch.nn.functional.pad(emit, (0, -n_states % 4)) if n_states % 4 else emit.contiguous()
    U = int(utt_ptr.shape[0]) - 1
    path = torch.empty(N, dtype=torch.int32, device=dev)
    score = torch.empty(U, dtype=torch.float32, device=dev)
    if U == 0:
        return path, score
    status = hip_ext.status_word(dev)
    need = int(lib.fhvae_vit_ws_bytes(N, n_states))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    out = path if N else torch.empty(1, dtype=torch.int32, device=dev)
    hb._call("fhvae_vit_decode", hb._p(emit), emit.stride(0), N, n_states, hb._p(trans), hb._p(init), hb._p(fin) if fin is not None else None,
             hb._p(utt_ptr), U, hb._p(out), hb._p(score), hb._p(status), hb._p(ws), ws.numel())
    if int(status.item()) & VIT_BAD_PTR:
        raise RuntimeError("%s: utt_ptr is not monotone from 0 to the %d rows of emit (nothing was written)" % (op, N))
    return path, score


def align(ref, ref_ptr, hyp, hyp_ptr):
    """fhvae_edit_align.  ref, hyp int32 tokens with their (U + 1,) int64 pointers, on the device -> counts (U, 4) int32:
    substitutions, deletions, insertions, correct.  One host sync, for the status word; a ref of more than 256 tokens raises."""
    import torch

    import hip_binding as hb

    op = "align"
    ref = _device(op, "ref", ref, torch.int32, 1).contiguous()
    hyp = _device(op, "hyp", hyp, torch.int32, 1).contiguous()
    ref_ptr, hyp_ptr = _ptr(op, "ref_ptr", ref_ptr), _ptr(op, "hyp_ptr", hyp_ptr)
    if ref_ptr.shape != hyp_ptr.shape:
        raise RuntimeError("%s: ref_ptr holds %d entries, hyp_ptr %d" % (op, ref_ptr.shape[0], hyp_ptr.shape[0]))
    load_library()
    U = int(ref_ptr.shape[0]) - 1
    counts = torch.empty(U, 4, dtype=torch.int32, device=ref.device)
    if U == 0:
        return counts
    if int(ref_ptr[-1]) > ref.shape[0] or int(hyp_ptr[-1]) > hyp.shape[0]:
        raise RuntimeError("%s: the pointers run past the %d / %d tokens" % (op, ref.shape[0], hyp.shape[0]))
    one = torch.zeros(1, dtype=torch.int32, device=ref.device)  # (an empty token array has no address)
    status = hip_ext.status_word(ref.device)
    hb._call("fhvae_edit_align", hb._p(ref if ref.numel() else one), hb._p(ref_ptr), hb._p(hyp if hyp.numel() else one), hb._p(hyp_ptr), U,
             hb._p(counts), hb._p(status))
    bits = int(status.item())
    if bits & EDIT_BAD_PTR:
        raise RuntimeError("%s: ref_ptr or hyp_ptr is not monotone from 0 (nothing was written)" % op)
    if bits & EDIT_BAD_REF:
        raise RuntimeError("%s: a reference holds more than %d tokens" % (op, EDIT_MAX_REF))
    return counts


# -------------------------------------------------------------------------------------------------------------------- model
def _host(a, dtype):
    return np.asarray(a.cpu() if hasattr(a, "cpu") else a).astype(dtype)


def transitions(labels, lengths, n_classes, smooth=1.0, penalty=0.0):
    """The frame-level phone bigram -> (trans (C, C) f32, init (C,) f32), numpy.  Float64 counts of the pairs of consecutive
    labelled frames within an utterance (an unlabelled frame, label < 0, breaks a pair) and of each utterance's first labelled
    frame; + smooth, row-normalised, log.  A row (or init) whose counts and smooth are all 0 is uniform.  `penalty` is subtracted
    from every off-diagonal entry of trans: the phone insertion penalty."""
    labels, lengths = _host(labels, np.int64), _host(lengths, np.int64)
    n_classes = int(n_classes)
    if labels.ndim != 1 or int(lengths.sum()) != labels.shape[0] or (lengths < 0).any():
        raise ValueError("transitions: %d labels for utterances of %d frames" % (labels.shape[0], int(lengths.sum())))
    if n_classes < 1 or (labels >= n_classes).any():
        raise ValueError("transitions: a label lies outside the %d classes" % n_classes)
    if not smooth >= 0:
        raise ValueError("transitions: smooth = %r must not be negative" % (smooth,))
    pair = np.zeros((n_classes, n_classes), dtype=np.float64)
    first = np.zeros(n_classes, dtype=np.float64)
    inner = np.ones(labels.shape[0], dtype=bool)  # frame i and i - 1 lie in one utterance
    base = np.concatenate([[0], np.cumsum(lengths)])
    inner[base[:-1][lengths > 0]] = False
    ok = inner[1:] & (labels[1:] >= 0) & (labels[:-1] >= 0) if labels.shape[0] > 1 else np.zeros(0, dtype=bool)
    np.add.at(pair, (labels[:-1][ok], labels[1:][ok]), 1.0)
    for a, b in zip(base[:-1], base[1:]):
        seg = labels[a:b]
        lab = seg[seg >= 0]
        if lab.shape[0]:
            first[lab[0]] += 1.0

    def logs(counts):
        c = counts + float(smooth)
        tot = c.sum(axis=-1, keepdims=True)
        c = np.where(tot > 0, c, 1.0)
        with np.errstate(divide="ignore"):
            return np.log(c / c.sum(axis=-1, keepdims=True))

    trans, init = logs(pair), logs(first)
    trans = trans - float(penalty) * (1.0 - np.eye(n_classes))
    return trans.astype(np.float32), init.astype(np.float32)


def emissions(x, model, priors=None, acoustic_scale=1.0, prior_scale=1.0, chunk=65536):
    """x (N, D) f32 on the device, a probe model -> (N, C) f32 on the device:
        acoustic_scale * (log_softmax(x @ tab.T + cst) - prior_scale * log priors)
    with (tab, cst) of probe.table; torch ops in row chunks.  priors (C,) float64 (default: none subtracted).  A class with bias
    -inf stays -inf whatever its prior.  This is by nature an (N, C) array: the decoder reads every score of every frame."""
    import torch

    import probe

    w, b, mean, std, _ = probe._model_arrays("emissions", model)
    x, D = probe._rows("emissions", "x", x)
    if D != w.shape[1]:
        raise ValueError("emissions: the rows have %d columns, the model %d" % (D, w.shape[1]))
    tab, cst = probe.table(w, b, mean, std, device=x.device)
    n_classes = int(tab.shape[0])
    sub = torch.zeros(n_classes, dtype=torch.float32, device=x.device)
    if priors is not None:
        pr = np.asarray(priors, dtype=np.float64)
        live = np.isfinite(b)
        if pr.shape != (n_classes,) or (pr[live] <= 0).any():
            raise ValueError("emissions: priors must be (%d,) and positive for every class the model can predict" % n_classes)
        sub = torch.from_numpy((float(prior_scale) * np.log(np.where(live, pr, 1.0))).astype(np.float32)).to(x.device)
    out = torch.empty(int(x.shape[0]), n_classes, dtype=torch.float32, device=x.device)
    dead = torch.isinf(cst) & (cst < 0)
    for a in range(0, int(x.shape[0]), int(chunk)):
        lp = torch.log_softmax(x[a:a + chunk] @ tab.T + cst[None, :], dim=1)
        lp = float(acoustic_scale) * (lp - sub[None, :])
        out[a:a + chunk] = torch.where(dead[None, :], torch.full_like(lp, float("-inf")), lp)
    return out


def _csr_keep(values, keep, ptr):
    """values[keep] with the pointers of the kept entries: (tokens int32, ptr int64), on the device of `values`."""
    import torch

    csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=values.device), torch.cumsum(keep.to(torch.int64), 0)])
    return values[keep].to(torch.int32).contiguous(), csum[ptr.to(torch.int64)].contiguous()


def collapse(path, utt_ptr):
    """path (N,) integers and utt_ptr (U + 1,) int64 on one device -> (tokens int32, ptr int64 (U + 1,)): every run of equal
    states within an utterance becomes one token.  Torch ops, no host sync."""
    import torch

    N = int(path.shape[0])
    keep = torch.ones(N, dtype=torch.bool, device=path.device)
    if N > 1:
        keep[1:] = path[1:] != path[:-1]
    starts = utt_ptr[:-1].to(torch.int64)
    keep[starts[starts < N]] = True
    return _csr_keep(path, keep, utt_ptr)


def fold(tokens, ptr, table):
    """Map token ids through an integer table (numpy or tensor): tokens[i] -> table[tokens[i]]; a target of -1 deletes the token.
    No merging afterwards: two neighbours that fold to the same phone stay two tokens.  The reference and the hypothesis are
    both mapped with this function.  -> (tokens int32, ptr int64)."""
    import torch

    table = torch.as_tensor(np.asarray(table.cpu() if hasattr(table, "cpu") else table), dtype=torch.int64).to(tokens.device)
    if tokens.numel() and (int(tokens.min()) < 0 or int(tokens.max()) >= table.shape[0]):
        raise ValueError("fold: a token lies outside the table's %d entries" % table.shape[0])
    mapped = table[tokens.to(torch.int64)]
    return _csr_keep(mapped, mapped >= 0, ptr)


def read_phone_map(path, names):
    """A phone map: lines `phone target`; a target `-` deletes the phone; a phone of `names` that is not listed maps to itself;
    a blank line or one that starts with '#' is skipped.  -> (table (len(names),) int32 into folded_names, -1 for a deleted phone;
    folded_names in order of first use).  A line without two fields or a phone listed twice raises ValueError naming the line."""
    target = {}
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            s = line.strip()
            if not s or s.startswith("#"):
                continue
            f = s.split()
            if len(f) != 2:
                raise ValueError("%s line %d: %d fields, not 'phone target'" % (path, no, len(f)))
            if f[0] in target:
                raise ValueError("%s line %d: phone '%s' is listed twice" % (path, no, f[0]))
            target[f[0]] = f[1]
    folded, index = [], {}
    table = np.empty(len(names), dtype=np.int32)
    for i, name in enumerate(names):
        t = target.get(name, name)
        if t == "-":
            table[i] = -1
            continue
        if t not in index:
            index[t] = len(folded)
            folded.append(t)
        table[i] = index[t]
    return table, folded


def references(items, keys):
    """Item lines (abx.read_items) -> for every utterance of `keys` the list of its tokens' phones in onset order (equal onsets:
    file order).  The frame grid plays no part: a token too short to own a frame is still a token of the transcription."""
    index = {k: i for i, k in enumerate(keys)}
    per = [[] for _ in keys]
    for no, (name, on, _, phone, _, _, _) in enumerate(items):
        u = index.get(name)
        if u is not None:
            per[u].append((on, no, phone))
    return [[p for _, _, p in sorted(toks)] for toks in per]


def error_rate(counts):
    """counts (U, 4): substitutions, deletions, insertions, correct -> {"per": (S + D + I) / (S + D + Cor), "sub", "del", "ins",
    "cor", "ref_tokens", "utterances"}; float64 / int on the host.  Without a reference token per is 0 (inf if something was
    inserted)."""
    c = _host(counts, np.int64).reshape(-1, 4)
    if (c < 0).any():
        raise ValueError("error_rate: a pair was refused by the aligner (counts of -1)")
    S, D, I, Cor = (int(v) for v in c.sum(axis=0))
    n = S + D + Cor
    per = (S + D + I) / float(n) if n else (0.0 if I == 0 else float("inf"))
    return {"per": per, "sub": S, "del": D, "ins": I, "cor": Cor, "ref_tokens": n, "utterances": int(c.shape[0])}


def csr(seqs, device=None):
    """A list of integer sequences -> (tokens int32, ptr int64) tensors."""
    import torch

    ptr = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    flat = np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs]) if len(seqs) and ptr[-1] else np.zeros(0, np.int32)
    return torch.from_numpy(flat.astype(np.int32)).to(device), torch.from_numpy(ptr).to(device)


def uncsr(tokens, ptr):
    """The inverse of csr, on the host: a list of int lists."""
    t, p = _host(tokens, np.int64), _host(ptr, np.int64)
    return [t[a:b].tolist() for a, b in zip(p[:-1], p[1:])]


def recognise(train_x, train_y, train_lengths, test_x, test_lengths, test_refs, names, l2=1e-4, iters=200, gtol=1e-5, model=None,
              smooth=1.0, penalty=0.0, acoustic_scale=1.0, prior_scale=1.0, phone_table=None, test_y=None):
    """What both command lines do.  train_x (N, D) f32, train_y (N,) labels (< 0: unlabelled), test_x on the device;
    train_lengths / test_lengths the frames per utterance; test_refs one list of ids into `names` per test utterance.
    Fit the probe on the training rows (or take `model`); priors = the labelled training class frequencies; transitions from the
    training labels; emissions of the test rows; viterbi; collapse; fold (phone_table, both sides); align.
    -> (model, report, hyp, ref): report = error_rate's keys plus per_argmax (the collapsed arg-max of probe.rows instead of the
    Viterbi path), frame_accuracy, frame_accuracy_argmax (None without test_y), classes and the settings; hyp / ref: the folded
    id lists per utterance."""
    import torch

    import probe

    n_classes = len(names)
    if n_classes < 1 or n_classes > VIT_MAX_STATES:
        raise ValueError("%d phones: the decoder takes 1 to %d states" % (n_classes, VIT_MAX_STATES))
    hist = {"iterations": 0, "converged": True}
    if model is None:
        model, hist = probe.fit(train_x, train_y, n_classes, l2=l2, iters=iters, gtol=gtol)
    elif probe._model_arrays("recognise", model)[0].shape != (n_classes, int(train_x.shape[1])):
        raise ValueError("the model has weights %s, the data %d classes of %d columns" % (model["weights"].shape, n_classes, train_x.shape[1]))
    dev = test_x.device
    ty = _host(train_y, np.int64)
    freq = np.bincount(ty[ty >= 0], minlength=n_classes).astype(np.float64)
    if freq.sum() == 0:
        raise ValueError("no training frame has a label")
    priors = freq / freq.sum()
    trans, init = transitions(ty, train_lengths, n_classes, smooth, penalty)
    emit = emissions(test_x, model, priors, acoustic_scale, prior_scale)
    utt_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(_host(test_lengths, np.int64))]).astype(np.int64)).to(dev)
    if int(utt_ptr[-1]) != int(test_x.shape[0]) or len(test_refs) != int(utt_ptr.shape[0]) - 1:
        raise ValueError("test_lengths and test_refs do not describe the %d test rows" % int(test_x.shape[0]))
    path, _ = viterbi(emit, utt_ptr, torch.from_numpy(trans).to(dev), torch.from_numpy(init).to(dev))
    w, b, mean, std, _ = probe._model_arrays("recognise", model)
    tab, cst = probe.table(w, b, mean, std, device=dev)
    none = torch.full((int(test_x.shape[0]),), -1, dtype=torch.int32, device=dev)
    pred = probe.rows(test_x, none, tab, cst)[1]
    table = np.arange(n_classes, dtype=np.int32) if phone_table is None else np.asarray(phone_table, dtype=np.int32)
    if table.shape != (n_classes,):
        raise ValueError("the phone table has %s entries for %d phones" % (table.shape, n_classes))
    ref_tok, ref_ptr = fold(*csr(test_refs, dev), table)
    report = {}
    for key, states in (("", path), ("_argmax", pred)):
        hyp_tok, hyp_ptr = fold(*collapse(states, utt_ptr), table)
        rates = error_rate(align(ref_tok, ref_ptr, hyp_tok, hyp_ptr))
        if key == "":
            report.update(rates)
            hyp = uncsr(hyp_tok, hyp_ptr)
        else:
            report["per_argmax"] = rates["per"]
        report["frame_accuracy" + key] = None
        if test_y is not None:
            tt = torch.as_tensor(table, dtype=torch.int64).to(dev)
            y = torch.as_tensor(test_y).to(dev).to(torch.int64)
            truth = torch.where(y >= 0, tt[y.clamp(min=0)], torch.full_like(y, -1))
            lab = truth >= 0
            n = int(lab.sum())
            report["frame_accuracy" + key] = float((tt[states.to(torch.int64)][lab] == truth[lab]).sum()) / n if n else 0.0
    report.update({"classes": list(names), "test_frames": int(test_x.shape[0]), "iterations": int(hist["iterations"]),
                   "converged": bool(hist["converged"]), "l2": float(l2), "smooth": float(smooth), "phone_penalty": float(penalty),
                   "acoustic_scale": float(acoustic_scale), "prior_scale": float(prior_scale)})
    return model, report, hyp, uncsr(ref_tok, ref_ptr)
