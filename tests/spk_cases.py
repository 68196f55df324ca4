"""The shared case table of tests/test_spk_cpu.py and tests/test_spk_gpu.py: per case a back end fitted by the oracle
(tests/spk_ref.py) on planted two-covariance training data, evaluation rows of held-out speakers, the f32 tables, the f32
rows v, a as the device holds them, and the oracle's per-class figures.  Everything comes from the oracle alone and is
computed once per process (lru_cache); the arrays are read-only."""
import functools

import numpy as np

import spk_ref as R

# name -> S evaluation rows, true width, NB, length normalisation, seed
SPECS = {
    "S1-w16": dict(S=1, width=16, NB=64, ln=False, seed=1),
    "S2-w16": dict(S=2, width=16, NB=64, ln=False, seed=2),
    "S63-w1": dict(S=63, width=1, NB=64, ln=False, seed=3),
    "S64-w5": dict(S=64, width=5, NB=256, ln=False, seed=4),
    "S65-w16": dict(S=65, width=16, NB=256, ln=True, seed=5),
    "S255-w24": dict(S=255, width=24, NB=4096, ln=True, seed=6),
    "S256-w32": dict(S=256, width=32, NB=4096, ln=False, seed=7),
    "S257-w5": dict(S=257, width=5, NB=64, ln=False, seed=8),
    "S777-w24": dict(S=777, width=24, NB=8192, ln=True, seed=9),
    "S777-w100": dict(S=777, width=100, NB=256, ln=False, seed=10),
    "S1100-w128": dict(S=1100, width=128, NB=8192, ln=False, seed=11),
}
NAMES = list(SPECS)
CAP = 0.0025  # at no edge may more than this share of a class's trials lie within delta of it


def _freeze(*arrays):
    for t in arrays:
        t.setflags(write=False)


@functools.lru_cache(maxsize=None)
def model(width, ln):
    """The oracle's fit on max(40, width + 30) planted speakers of about 20 rows, `width` columns (no LDA: the PLDA alone; the
    between-class covariance has full rank, so the oracle may invert it) -> (fit dict, tables)."""
    x, label = R.planted(100 + width, max(40, width + 30), 20, width)
    m = R.fit(x, label, None, ln, iters=5)
    return m, R.tables(m)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: spec fields, x (S, width) f32, label (S,) int32, tab (the f32 tables), v (S, Dp) f32, a (S,) f32, c, and i, j,
    same (the trials), s, M (float64 score and magnitude per trial)."""
    spec = SPECS[name]
    S, width = spec["S"], spec["width"]
    speakers = max(2, S // 25)
    x, label = R.planted(1000 + spec["seed"], speakers, 25, width)
    while len(label) < S:  # (Poisson counts: draw more speakers until there are S rows)
        speakers += 2
        x, label = R.planted(1000 + spec["seed"], speakers, 25, width)
    x, label = np.ascontiguousarray(x[:S]), np.ascontiguousarray(label[:S])
    _, tab = model(width, spec["ln"])
    v, a = R.transform32(tab, x, spec["ln"])
    i, j, same = R.trials(label)
    s, M = R.scores(v, a, tab["c"], i, j)
    _freeze(x, label, v, a, i, j, same, s, M)
    return dict(spec, name=name, x=x, label=label, tab=tab, v=v, a=a, c=tab["c"], Dp=v.shape[1], i=i, j=j, same=same, s=s, M=M)


def score_range(c):
    """The oracle's (lo, hi) of a case as f32 values (what the test hands the oracle is the kernel's own; this one serves the
    CPU check of the cap)."""
    if len(c["s"]) == 0:
        return 0.0, 0.0
    return float(np.float32(c["s"].min())), float(np.float32(c["s"].max()))


def classes(c, lo, hi):
    """Per class (0 target, 1 non-target): (s, delta, cum, near, hist) over [lo, hi) in the case's NB bins."""
    out = []
    for cls in (True, False):
        sel = c["same"] == cls
        s, dlt = c["s"][sel], R.delta(c["M"][sel], c["Dp"], lo, hi)
        cum, near, hist = R.edge_counts(s, dlt, lo, hi, c["NB"])
        out.append((s, dlt, cum, near, hist))
    return out


def worst_edge(c):
    """-> per class (most trials within delta of one edge, trials of the class), from the oracle alone."""
    lo, hi = score_range(c)
    return [(int(near.max()) if len(s) else 0, len(s)) for s, _, _, near, _ in classes(c, lo, hi)]
