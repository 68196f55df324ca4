"""What the GPU tests of the sequence-trellis kernels share to build and compare their cases: tests/test_ctc_gpu.py,
tests/test_falign_gpu.py, tests/test_ctcbeam_gpu.py and tests/test_phonerec_gpu.py.  A plain module, as tests/ctcbeam_cases.py
and tests/glue_cases.py.  (ctcbeam_cases.ptr_of takes a case dict; the one here takes the lengths.)
"""
import numpy as np


def dev(a):
    """A host array as a contiguous tensor on the device."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr_of(lengths):
    """Lengths per utterance -> the (U + 1,) int64 pointer array from 0."""
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def bits64(a):
    """The bits of a float64 (or int64) array or tensor, as int64."""
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.int64)


def bits32(a):
    """The bits of an f32 (or int32) array or tensor, as int32."""
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.int32)


def labels_for(rng, L, C, blank, repeats):
    """L labels without the blank, neighbours different where C allows, then `repeats` neighbours made equal."""
    classes = [c for c in range(C) if c != blank]
    lab = []
    for _ in range(L):
        pick = [c for c in classes if not lab or c != lab[-1]] or classes
        lab.append(int(pick[rng.integers(len(pick))]))
    for i in rng.permutation(max(L - 1, 0))[:repeats]:
        lab[i + 1] = lab[i]
    return lab


def blank_of(C, where):
    """The blank's class by name; "hmm" is the topology without one (-1)."""
    return {"first": 0, "middle": C // 2, "last": C - 1, "hmm": -1}[where]
