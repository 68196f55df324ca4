"""The cases tests/test_segment_gpu.py runs on the device and tests/test_segment_cpu.py checks beforehand with the oracle alone
(the share of cells whose runner-up lies within 2 B of the best must stay under 1 % by construction).  A plain module, as
tests/ctcbeam_cases.py."""
import functools

import numpy as np

import segment_ref as R

LAMBDAS = (0.0, 0.25, 4.0)


def lengths_for(L):
    """T in {0, 1, 2, Lmax - 1, Lmax, Lmax + 1, 63, 64, 65, 300}, in an order that puts the empty utterance inside the batch."""
    return [1, 2, 0, max(L - 1, 0), L, L + 1, 63, 64, 65, 300]


def _specs():
    specs = {}
    i = 0
    for L in (1, 2, 5, 32, 64):
        for K in (1, 2, 17, 65):
            # the layouts rotate over the sweep: a padded leading dimension of x, a strided view of the codebook
            specs["L%d_K%d" % (L, K)] = dict(L=L, K=K, D=32, lengths=lengths_for(L), pad_x=i % 2 == 1, stride_c=i % 3 == 1, seed=100 + i)
            i += 1
    specs["D16"] = dict(L=5, K=17, D=16, lengths=[0, 1, 6, 65, 300], pad_x=True, stride_c=False, seed=201)
    specs["D80"] = dict(L=32, K=2, D=80, lengths=[31, 0, 33, 65, 300], pad_x=False, stride_c=True, seed=202)
    specs["D128"] = dict(L=64, K=65, D=128, lengths=[63, 65, 0, 1, 300], pad_x=True, stride_c=True, seed=203)
    specs["one_T300"] = dict(L=5, K=17, D=32, lengths=[300], pad_x=False, stride_c=False, seed=204)
    specs["one_T1"] = dict(L=32, K=65, D=32, lengths=[1], pad_x=True, stride_c=False, seed=205)
    specs["mixed7"] = dict(L=32, K=17, D=32, lengths=[17, 0, 300, 1, 64, 5, 129], pad_x=False, stride_c=True, seed=206)
    # more rows than a chunk of segment sums holds (4096) with an utterance across the edge, and an utterance longer than a
    # trace-back window (2048)
    specs["long"] = dict(L=5, K=2, D=32, lengths=[4090, 10, 300], pad_x=False, stride_c=False, seed=207)
    return specs


SPECS = _specs()
NAMES = list(SPECS)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: x (N, D) f32, cent (K, D) f32, lengths, ptr (U + 1,) int64, L, pad_x, stride_c and the oracle's score64, unit, gap,
    B (N, L) over the batch.  Standard normal rows and centroids: the scores of two units differ by something of order 1, B is of
    order 1e-4.  Computed once and shared; the tests leave it unchanged."""
    sp = SPECS[name]
    rng = np.random.default_rng(sp["seed"])
    lengths = np.asarray(sp["lengths"], dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    x = rng.standard_normal((int(ptr[-1]), sp["D"])).astype(np.float32)
    cent = rng.standard_normal((sp["K"], sp["D"])).astype(np.float32)
    score, unit, gap, B = R.batch_scores(x, cent, ptr, sp["L"])
    out = dict(sp, name=name, x=x, cent=cent, lengths=lengths, ptr=ptr, score=score, unit=unit, gap=gap, B=B)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def inside_gap(c):
    """The share of the case's finite cells whose runner-up lies within 2 B of the best."""
    fin = np.isfinite(c["score"])
    return float((c["gap"][fin] <= 2 * c["B"][fin]).mean()) if fin.any() else 0.0
