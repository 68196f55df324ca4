"""verification.py -- speaker verification on embeddings: does the factorization work?

Every sequence is scored against every other by the cosine of their embeddings (the FHVAE papers use the per-sequence mu2, and
the per-sequence mean of z1 as the control); a trial is a target when both sequences have the same speaker.  The equal error
rate (EER) is where the share of non-targets accepted equals the share of targets rejected: low on mu2 and high on z1 for a
model that separated the speaker from the content.

The all-pairs scoring is one HIP kernel (hip_binding.sv_hist: no (S, S) score matrix) that returns the two classes' score
histograms; the EER is read off the histograms on the host (eer_from_hist, numpy only).
"""
from __future__ import annotations

from itertools import accumulate

import numpy as np


def eer_from_hist(hist) -> dict:
    """hist (2, NB) counts, row 0 target and row 1 non-target trials, bin b = scores in [-1 + 2b/NB, -1 + 2(b+1)/NB).

    For edge k in 0..NB a trial is accepted iff its bin >= k: FAR(k) the share of non-targets accepted, FRR(k) the share of
    targets rejected.  The EER is the linear interpolation between edges k - 1 and k at the first k with FRR(k) >= FAR(k).
    -> eer, threshold (the interpolated score), n_target, n_nontarget, crossing_mass (the share of targets plus the share of
    non-targets in bin k - 1: what one bin can hide, the resolution of this EER)."""
    h = np.asarray(hist)
    if h.ndim != 2 or h.shape[0] != 2 or h.shape[1] < 1:
        raise ValueError("eer_from_hist takes a (2, NB) histogram, got shape %s" % (h.shape,))
    tar, non = [[int(v) for v in row] for row in h]  # (Python integers: uint64 counts do not wrap)
    nb = len(tar)
    n_tar, n_non = sum(tar), sum(non)
    if n_tar == 0:
        raise ValueError("no target trials: no two labelled sequences share a speaker")
    if n_non == 0:
        raise ValueError("no non-target trials: all labelled sequences have the same speaker")
    frr = np.array([r / n_tar for r in [0] + list(accumulate(tar))], dtype=np.float64)  # targets in bins < k
    far = np.array([(n_non - b) / n_non for b in [0] + list(accumulate(non))], dtype=np.float64)  # non-targets in bins >= k
    k = int(np.argmax(frr >= far))  # FRR(0) = 0 < FAR(0) = 1 and FRR(NB) = 1 > FAR(NB) = 0: 1 <= k <= NB
    d0, d1 = frr[k - 1] - far[k - 1], frr[k] - far[k]  # d0 < 0 <= d1
    t = -d0 / (d1 - d0)
    eer = frr[k - 1] + t * (frr[k] - frr[k - 1])
    return {"eer": float(eer), "threshold": float(-1.0 + 2.0 * (k - 1 + t) / nb), "n_target": n_tar, "n_nontarget": n_non,
            "crossing_mass": tar[k - 1] / n_tar + non[k - 1] / n_non}


def speaker_verification(emb, labels, n_bins: int = 4096, device=None) -> dict:
    """emb (S, D) embeddings (array or tensor), labels (S,) integers, -1 = unlabelled (the row takes part in no trial)
    -> eer_from_hist's dict plus "hist", the (2, n_bins) int64 numpy histogram.  Scoring runs on the GPU (no CPU fallback)."""
    import torch

    import hip_binding as hb

    if device is None:
        device = emb.device if isinstance(emb, torch.Tensor) and emb.is_cuda else torch.device("cuda:0")
    if not isinstance(emb, torch.Tensor):
        emb = torch.from_numpy(np.array(emb, dtype=np.float32))  # (a copy: read-only arrays and views are welcome)
    e = emb.to(device=device, dtype=torch.float32)
    lab = torch.as_tensor(np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).astype(np.int32)).to(device)
    if e.dim() != 2 or lab.dim() != 1 or lab.shape[0] != e.shape[0]:
        raise ValueError("speaker_verification takes (S, D) embeddings and (S,) labels")
    hist = hb.sv_hist(e, lab, n_bins).cpu().numpy()
    out = eer_from_hist(hist)
    out["hist"] = hist
    return out


def read_utt2spk(path) -> dict:
    """Kaldi's utt2spk: one `<seq> <spk>` per line -> {seq: spk}."""
    table = {}
    with open(path) as f:
        for n, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != 2:
                raise ValueError("%s:%d: expected `<seq> <spk>`, got %r" % (path, n, line.rstrip("\n")))
            if parts[0] in table:
                raise ValueError("%s:%d: sequence %r is listed twice" % (path, n, parts[0]))
            table[parts[0]] = parts[1]
    return table


def speakers_from_keys(keys, sep: str) -> list:
    """The speaker of every key = the key up to the first `sep`: "-" for preprocess_librispeech.py's ids
    (<speaker>-<chapter>-<utt>), "_" for preprocess_timit.py's (<speaker>_<name>)."""
    if not sep:
        raise ValueError("the separator is empty")
    out = []
    for key in keys:
        head, found, _ = str(key).partition(sep)
        if not found or not head:
            raise ValueError("key %r has no speaker in front of a %r" % (key, sep))
        out.append(head)
    return out


def labels_from_speakers(speakers):
    """speakers: one name per sequence, None = unknown -> ((S,) int32 labels with -1 for None, number of speakers)."""
    names = sorted({s for s in speakers if s is not None})
    index = {s: i for i, s in enumerate(names)}
    return np.asarray([-1 if s is None else index[s] for s in speakers], dtype=np.int32), len(names)
