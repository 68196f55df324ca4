"""The shared case table of tests/test_snorm_cpu.py and tests/test_snorm_gpu.py.  Everything comes from the oracles alone
(tests/snorm_ref.py, tests/spk_ref.py, tests/spk_cases.py) and is computed once per process (lru_cache); the arrays are read-only.

  STATS   cohort statistics: random f32 rows of a true width (zero-padded to a multiple of 16), S evaluation rows against Nc
          cohort rows, the top K
  EXACT   integer-valued cohort statistics: entries in -2 .. 2, integer a, az and c, so every score is exact in f32
  PAIRS   the normalised score of all pairs: rows of tests/spk_cases.py with a cohort of the same model
"""
import functools

import numpy as np

import snorm_ref as N
import spk_cases as SC
import spk_ref as R

# name -> S, Nc, true width, top, seed.  Together: S in 1, 63 / 64 / 65, 255 / 256 / 257, 600; Nc in 1, 2, 15 / 16 / 17, 63 / 64 / 65,
# 129, 1000; widths 1, 5, 16, 24, 48, 100, 128; top in 0, 1, 2, Nc - 1, Nc, Nc + 5, 20
STATS = {
    "S1-Nc1-w16-top0": dict(S=1, Nc=1, width=16, top=0, seed=1),
    "S63-Nc2-w1-top1": dict(S=63, Nc=2, width=1, top=1, seed=2),
    "S64-Nc15-w5-top2": dict(S=64, Nc=15, width=5, top=2, seed=3),
    "S65-Nc16-w16-top15": dict(S=65, Nc=16, width=16, top=15, seed=4),
    "S255-Nc17-w24-top17": dict(S=255, Nc=17, width=24, top=17, seed=5),
    "S256-Nc63-w48-top68": dict(S=256, Nc=63, width=48, top=68, seed=6),
    "S257-Nc64-w100-top20": dict(S=257, Nc=64, width=100, top=20, seed=7),
    "S600-Nc65-w128-top0": dict(S=600, Nc=65, width=128, top=0, seed=8),
    "S65-Nc129-w24-top20": dict(S=65, Nc=129, width=24, top=20, seed=9),
    "S64-Nc129-w5-top1": dict(S=64, Nc=129, width=5, top=1, seed=10),
    "S257-Nc1000-w48-top20": dict(S=257, Nc=1000, width=48, top=20, seed=11),
    "S600-Nc1000-w16-top0": dict(S=600, Nc=1000, width=16, top=0, seed=12),
}
STATS_NAMES = list(STATS)

# name of a case of tests/spk_cases.py -> the cohort's speakers and the top K
PAIRS = {
    "S2-w16": dict(speakers=6, top=0),
    "S63-w1": dict(speakers=8, top=20),
    "S65-w16": dict(speakers=8, top=20),
    "S257-w5": dict(speakers=8, top=0),
    "S777-w24": dict(speakers=10, top=20),
    "S777-w100": dict(speakers=10, top=50),
    "S1100-w128": dict(speakers=10, top=20),
}
PAIRS_NAMES = list(PAIRS)
SD_FLOOR = 1e-6


def _freeze(*arrays):
    for t in arrays:
        t.setflags(write=False)


def _padded(x):
    out = np.zeros((x.shape[0], (x.shape[1] + 15) // 16 * 16), dtype=np.float32)
    out[:, :x.shape[1]] = x
    return out


@functools.lru_cache(maxsize=None)
def stats_case(name):
    """-> dict: the spec, v (S, Dp), a (S,), z (Nc, Dp), az (Nc,) f32, c, and the oracle's s (S, Nc), eps, thr, mu, sd (float64)."""
    spec = STATS[name]
    rs = np.random.RandomState(500 + spec["seed"])
    S, Nc, w = spec["S"], spec["Nc"], spec["width"]
    v = _padded((rs.randn(S, w) * rs.uniform(0.2, 3.0, size=(S, 1))).astype(np.float32))
    z = _padded((rs.randn(Nc, w) + 0.5).astype(np.float32))
    a, az = rs.randn(S).astype(np.float32), (2.0 * rs.randn(Nc)).astype(np.float32)
    c = float(np.float32(0.3))
    s, eps = N.cohort_scores(v, a, z, az, c)
    thr, mu, sd = N.stats(s, spec["top"])
    _freeze(v, a, z, az, s, eps, thr, mu, sd)
    return dict(spec, name=name, v=v, a=a, z=z, az=az, c=c, s=s, eps=eps, thr=thr, mu=mu, sd=sd)


def exact_case(kind):
    """Integer-valued operands -> (v, a, z, az, c, top): every score is an integer of small magnitude, exact in f32."""
    rs = np.random.RandomState({"ties": 1, "equal": 2, "negative": 3, "mixed": 4, "zero": 5}[kind])
    S, D = 70, 16
    v = rs.randint(-2, 3, size=(S, D)).astype(np.float32)
    a = rs.randint(-3, 4, size=S).astype(np.float32)
    if kind == "ties":       # 200 cohort rows, 3 distinct ones: K = 50 falls inside a tie
        base = rs.randint(-2, 3, size=(3, D)).astype(np.float32)
        pick = rs.randint(0, 3, size=200)
        return v, a, base[pick], np.array([1.0, -2.0, 0.0], np.float32)[pick], 2.0, 50
    if kind == "equal":      # all cohort rows equal: sd is at the floor
        return v, a, np.repeat(rs.randint(-2, 3, size=(1, D)).astype(np.float32), 40, axis=0), np.full(40, 3.0, np.float32), -1.0, 7
    z = rs.randint(-2, 3, size=(90, D)).astype(np.float32)
    az = rs.randint(-3, 4, size=90).astype(np.float32)
    if kind == "negative":   # |dot| <= 64 and |a + az| <= 6: every score is negative
        return v, a, z, az, -100.0, 20
    if kind == "mixed":
        return v, a, z, az, 0.0, 20
    # scores of zero: half the evaluation rows and a third of the cohort are zero rows with zero terms
    v[::2], a[::2] = 0.0, 0.0
    z[::3], az[::3] = 0.0, 0.0
    return v, a, z, az, 0.0, 45


EXACT_KINDS = ["ties", "equal", "negative", "mixed", "zero"]


@functools.lru_cache(maxsize=None)
def cohort(name):
    """The cohort of a pairs case: rows of other speakers of the case's model, through the oracle's f32 transform -> (z, az)."""
    c = SC.case(name)
    xc, _ = R.planted(2000 + c["seed"], PAIRS[name]["speakers"], 12, c["width"])
    z, az = R.transform32(c["tab"], xc, c["ln"])
    _freeze(z, az)
    return z, az


@functools.lru_cache(maxsize=None)
def oracle_stats(name):
    """(mu, r) f32 of a pairs case from the oracle alone (the GPU tests use the device's own; this serves the CPU check)."""
    c = SC.case(name)
    z, az = cohort(name)
    s, _ = N.cohort_scores(c["v"], c["a"], z, az, c["c"])
    _, mu, sd = N.stats(s, PAIRS[name]["top"])
    sd32 = np.maximum(sd.astype(np.float32), np.float32(SD_FLOOR))
    return mu.astype(np.float32), (np.float32(1) / sd32).astype(np.float32)


def classes(c, mu, r, lo, hi, NB=None):
    """Per class (0 target, 1 non-target) of the spk_cases case c with the f32 statistics mu, r: (sn, Delta, cum, near, hist)
    over [lo, hi) in NB bins (the case's unless given)."""
    out = []
    for cls in (True, False):
        sel = c["same"] == cls
        i, j, s, M = c["i"][sel], c["j"][sel], c["s"][sel], c["M"][sel]
        sn = N.normalise(s, mu, r, i, j)
        dlt = N.norm_delta(s, M, c["Dp"], mu, r, i, j, lo, hi)
        out.append((sn, dlt) + R.edge_counts(sn, dlt, lo, hi, c["NB"] if NB is None else NB))
    return out


def score_range(c, mu, r):
    """The oracle's (lo, hi) of the normalised scores as f32 values."""
    sn = N.normalise(c["s"], mu, r, c["i"], c["j"])
    return float(np.float32(sn.min())), float(np.float32(sn.max()))
