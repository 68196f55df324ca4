"""The shared case table and the seeded generators of the i-vector tests (tests/test_ivector_cpu.py, tests/test_ivector_gpu.py).
A plain module, as tests/spk_cases.py."""
import numpy as np

import ivector_ref as R

LENGTHS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 2049)  # around the MFMA's 4 and the trip's 16 rows, around one and two slices

#: name -> (utterance lengths, C, D, extra leading dimension of x and post).  Every length, every U in 1, 2, 9, every C and every Dp
#: of the issue appear; the C cases run at the smallest width, the wide ones at one C off the tile of 64
STATS_CASES = {
    "all_lengths": ((1025, 0, 16, 2049, 1, 1023, 17, 15, 1024), 17, 39, 0),
    "c1": ((17, 1025), 1, 5, 0),
    "c15": ((17, 1025), 15, 5, 0),
    "c16": ((17, 1025), 16, 8, 0),
    "c63": ((17, 1025), 63, 5, 0),
    "c64": ((17, 1025), 64, 5, 0),
    "c65": ((2049,), 65, 60, 0),
    "c130": ((1025, 17), 130, 5, 0),
    "ld": ((1024, 33), 17, 39, 8),
    "one": ((1,), 3, 40, 0),
}

#: (R, U): every rank of the issue and every U; 32 / 33 and 64 / 65 are where the kernel changes its threads per utterance
SOLVE_CASES = ((1, 70), (2, 3), (7, 3), (8, 1), (9, 3), (31, 3), (32, 70), (33, 70), (64, 3), (65, 3), (100, 3), (127, 1), (128, 3))


def stats_inputs(seed, lengths, C, D):
    """-> (x (N, D) f32, post (N, C) f32 rows that sum to about 1, ptr (U + 1,) int64)."""
    rng = np.random.default_rng(seed)
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    N = max(int(ptr[-1]), 1)
    x = (rng.standard_normal((N, D)) * 3.0 + 1.0).astype(np.float32)
    g = rng.random((N, C)) ** 4
    g[rng.random((N, C)) < 0.3] = 0.0
    g[np.arange(N), rng.integers(0, C, N)] += 0.5
    post = (g / g.sum(axis=1, keepdims=True)).astype(np.float32)
    return x, post, ptr


def solve_inputs(seed, R_, U, C=12, Dp=8):
    """L_u = I + sum_c n_c(u) T_c^T T_c of random T and counts, b random -> (L (U, R, R), b (U, R)).  T is N(0, 0.5^2) and n
    uniform below 40, which gives kappa_2 from about 2 at small ranks to 3 10^3 at R = 128.  At R = 1 the matrix is a number, kappa_2 = 1, and the bound on logdet is
    2^-52 ABSOLUTE: no float64 result of 4 or more can meet it (half a unit in the last place is 2^-51 there), so at R = 1 T is
    N(0, 0.07^2) and n below 10, which keeps L below e^2."""
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((C, Dp, R_)) * (0.07 if R_ == 1 else 0.5)
    n = rng.random((U, C)) * (10.0 if R_ == 1 else 40.0)
    L = np.stack([R.precision(n[u], T) for u in range(U)])
    b = rng.standard_normal((U, R_)) * 5.0
    return L, b


def planted(seed=3, C=8, D=5, speakers=24, per_speaker=10, frames=120, rank=3, session=0.35):
    """The planted set of the issue: C = 8, D = 5, 240 utterances of 120 frames from 24 speakers, a true rank of 3.
    Frame t of utterance u: a component c drawn by the weights, x = m_c + s_c (Tt_c w_u + e), e standard normal, with
    w_u = y_speaker + session * standard normal.  -> dict(x f32, ptr, labels, ubm)."""
    rng = np.random.default_rng(seed)
    ubm = {"weights": rng.dirichlet(np.full(C, 5.0)), "means": rng.standard_normal((C, D)) * 3.0,
           "variances": 0.5 + rng.random((C, D))}
    Tt = rng.standard_normal((C, D, rank)) * 0.45
    y = rng.standard_normal((speakers, rank))
    labels = np.repeat(np.arange(speakers), per_speaker)
    U = labels.shape[0]
    rows = []
    for u in range(U):
        w = y[labels[u]] + session * rng.standard_normal(rank)
        c = rng.choice(C, size=frames, p=ubm["weights"])
        off = np.einsum("tdr,r->td", Tt[c], w)
        rows.append(ubm["means"][c] + np.sqrt(ubm["variances"][c]) * (off + rng.standard_normal((frames, D))))
    x = np.concatenate(rows).astype(np.float32)
    ptr = np.arange(U + 1, dtype=np.int64) * frames
    for a in (x, ptr, labels):
        a.setflags(write=False)
    return {"x": x, "ptr": ptr, "labels": labels, "ubm": ubm}


_cache = {}


def planted_stats():
    """The planted set with its float64 posteriors rounded to f32 (the `post` both the oracle and the device sum), the oracle's
    float64 statistics of them and their bounds; computed once."""
    if "p" not in _cache:
        p = dict(planted())
        p["post"] = R.posteriors(p["x"], p["ubm"]).astype(np.float32)
        p["n"], p["f"], an, af = R.stats64(p["x"], p["post"], p["ptr"])
        p["dn"], p["df"] = R.stats_bound(p["n"], p["f"], an, af)
        p["ft"] = R.whiten(p["n"], p["f"], p["ubm"])
        for v in p.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache["p"] = p
    return _cache["p"]


def planted_em(min_div):
    """The oracle's EM on the planted set, 3 iterations at R = 3 from the start of seed 0; computed once per flag."""
    key = ("em", bool(min_div))
    if key not in _cache:
        p = planted_stats()
        C, D = p["ubm"]["means"].shape
        _cache[key] = R.em(p["n"], p["ft"], R.start(C, D, 3, 0), 3, min_div)
    return _cache[key]
