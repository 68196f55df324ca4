"""The inputs that tests/test_ctcbeam_cpu.py vets with the oracle and tests/test_ctcbeam_gpu.py runs on the device: one generator,
so the CPU test's margin condition covers exactly what the GPU test compares.  A plain module, as tests/glue_cases.py.

A case is a dict: name, C, blank, W, scale, class_beam, table ((C + 1, C + 1) float64 or None), lengths (frames per utterance,
empty ones between the others), z ((N, C) f32).  oracle(case) runs tests/ctcbeam_ref.py on it once per process.
"""
import functools

import numpy as np

import ctcbeam_ref as R

CLASSES = (2, 3, 5, 61, 64, 65, 128)
BEAMS = (1, 2, 3, 16, 63, 64)
LENGTHS = (0, 1, 2, 63, 64, 65, 130, 300)
SCALES = (1.0, 50.0)

#: case name -> the seed that replaces the default 0 (a seed whose oracle margin fails the condition of test_ctcbeam_cpu.py is
#: replaced here, on the CPU, before anything runs on a GPU)
SEEDS = {}


def bound(T, score):
    """The score bound of the GPU test: 5 T 2^-53 max(1, |score|)."""
    return 5.0 * T * 2.0 ** -53 * max(1.0, abs(score))


def _make(name, C, blank, W, scale, class_beam, with_table, lengths):
    import zlib

    rng = np.random.default_rng([zlib.crc32(name.encode()), SEEDS.get(name, 0)])
    z = (scale * rng.standard_normal((int(sum(lengths)), C))).astype(np.float32)
    table = rng.standard_normal((C + 1, C + 1)) if with_table else None
    return {"name": name, "C": C, "blank": blank, "W": W, "scale": scale, "class_beam": class_beam, "table": table,
            "lengths": list(lengths), "z": z}


def _grid_params():
    k = 0
    for C in CLASSES:
        for W in BEAMS:
            blank = (0, C // 2, C - 1)[k % 3]
            scale = SCALES[(k // 3) % 2]
            with_table = (k // 2) % 2 == 1
            class_beam = 2.5 * scale if (k // 4) % 2 == 1 else np.inf
            if W * C >= 1024:  # the oracle is slow here: two utterances, an empty one between them
                lengths = (LENGTHS[1 + k % 7], 0, LENGTHS[3 + k % 5])
            else:
                lengths = (0, 1, 2, 0, 63, 64, 65, 0, 130, 300, 0)
            yield "grid-C%d-W%d" % (C, W), C, blank, W, scale, class_beam, with_table, lengths
            k += 1


GRID = [p[0] for p in _grid_params()]


@functools.lru_cache(maxsize=None)
def case(name):
    for p in _grid_params():
        if p[0] == name:
            return _make(*p)
    if name.startswith("recreate-"):  # the regime in which a prefix falls out, its child stays and its parent makes it again
        return _make(name, 5, 4, 64, 1.0, np.inf, name.endswith("-lm"), (130,) * 6)
    if name == "never-fills":
        return _make(name, 2, 0, 64, 1.0, np.inf, False, (3, 3, 1, 2))
    raise KeyError(name)


RECREATE = ["recreate-plain", "recreate-lm"]
ALL = GRID + RECREATE + ["never-fills"]


def ptr_of(c):
    return np.concatenate([[0], np.cumsum(c["lengths"])]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(hyps, scores, margins, status, stats) of the oracle on case `name`."""
    c = case(name)
    ptr = ptr_of(c)
    hyps, scores, margins, stats, status = [], [], [], {"recreated": 0}, 0
    for u in range(len(c["lengths"])):
        h, s, m, emptied = R.decode(c["z"][ptr[u]:ptr[u + 1]], c["blank"], c["W"], c["table"], c["class_beam"], stats)
        hyps.append(h), scores.append(s), margins.append(m)
        status |= R.EMPTY if emptied else 0
    return hyps, np.array(scores), np.array(margins), status, stats


def small(with_table, seed=3):
    """T <= 5, C <= 3: (z, blank, table) for the brute-force tests."""
    rng = np.random.default_rng(seed + (100 if with_table else 0))
    for T in range(0, 6):
        for C in (2, 3):
            for blank in range(C):
                for rep in range(2):
                    z = (rng.standard_normal((T, C)) * (1.0 if rep == 0 else 3.0)).astype(np.float32)
                    yield z, blank, (rng.standard_normal((C + 1, C + 1)) if with_table else None)
