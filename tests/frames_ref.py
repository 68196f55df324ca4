"""numpy oracle of the two definitions of include/fhvae_frames.h, written as plain loops over windows and frames with no formula
shared with pytorch-scalablefhvae_amd/frames.py: which windows cover a frame is found by enumeration, not by the closed form.
float32 arithmetic in the stated order, one rounding per operation.  Shared by test_frames_cpu.py and test_frames_gpu.py."""
import numpy as np

F32 = np.float32


def n_windows(n, shift):
    return (n + shift - 1) // shift


def windows(feats, T, shift, mean=None, inv_std=None):
    """feats: list of (n_u, F) float32 arrays -> (total windows, T, F): window k of an utterance is centred on frame k * shift,
    position t reads frame min(max(k * shift - T // 2 + t, 0), n - 1); then (x - mean) * inv_std."""
    out = []
    for x in feats:
        n = x.shape[0]
        for k in range(n_windows(n, shift)):
            w = np.empty((T, x.shape[1]), F32)
            for t in range(T):
                p = k * shift - T // 2 + t
                w[t] = x[min(max(p, 0), n - 1)]
            out.append(w)
    out = np.stack(out).astype(F32)
    if mean is not None:
        out = ((out - mean.astype(F32)) * inv_std.astype(F32)).astype(F32)
    return out


def brute_covering(f, n, T, shift):
    """The windows of an n-frame utterance that hold local frame f at a position inside [0, T), by enumeration."""
    return [k for k in range(n_windows(n, shift)) if 0 <= f - (k * shift - T // 2) < T]


def overlap_mean(seg, lengths, T, shift, mean=None, std=None):
    """seg (total windows, T, F) float32, the windows of every utterance in order -> (total frames, F): frame f the sum, in
    increasing k, of seg[k, f - (k * shift - T // 2)] over the windows that cover it, one division by their number, then
    * std + mean."""
    rows, w_off = [], 0
    for n in lengths:
        for f in range(n):
            ks = brute_covering(f, n, T, shift)
            assert ks and ks == list(range(ks[0], ks[-1] + 1))
            acc = seg[w_off + ks[0], f - (ks[0] * shift - T // 2)].astype(F32)
            for k in ks[1:]:
                acc = (acc + seg[w_off + k, f - (k * shift - T // 2)]).astype(F32)
            acc = (acc / F32(len(ks))).astype(F32)
            if mean is not None:
                acc = ((acc * std.astype(F32)).astype(F32) + mean.astype(F32)).astype(F32)
            rows.append(acc)
        w_off += n_windows(n, shift)
    return np.stack(rows)
