"""The LSTM schedule queries (fhvae_lstm_form, _layout_id, _pre_elems, _ws_below_elems, _infer_cs_elems, _lp_bytes) over a sweep
of descriptors and schedule switches, and tests/golden/lstm_plan.json, which pins what they returned before the schedule was
decided by one plan (csrc/lstm_cluster.h, LstmPlan).  No query dereferences a pointer of the descriptor: the sweep hands them a
fake aligned address.

    python tests/lstm_plan_sweep.py --record      (on a MI355X: the persistent forms need the device check to pass)

The table has 16800 x 18 rows of six numbers, so the file holds it as digests: per switch setting one SHA-256 (16 hex digits)
for every block of 350 consecutive cases, i.e. one (dtype, lp, H, L) over all B, T and (I, Ic); and per switch setting a census
of the (form, layout) pairs, for a reader.  A block that differs is named by the tests with its first differing rows; the
numbers behind a digest come back from --record on the commit that recorded it.
"""
import collections
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lstm_plan.json")

DTYPES = (0, 1)  # hip_binding.F32, BF16
LPS = (False, True)
HS = (64, 128, 256, 512)
LS = (1, 2, 3)
BS = (16, 256, 1024, 1040, 2048, 4096, 8192, 16384, 131072, 131088)  # both forms, both chunk counts, the 32-bit bound
TS = (1, 4, 20, 4093, 4094)  # T + L against the flag epochs of a launch
IIC = ((80, 32), (80, 0), (0, 64), (84, 32), (136, 0), (0, 136), (80, 4))
SWITCHES = ("FHVAE_NO_CLUSTER", "FHVAE_NO_FOLD", "FHVAE_NO_XC_FOLD", "FHVAE_NO_FWD_WR", "FHVAE_NO_RS", "FHVAE_NO_WGRAD",
            "FHVAE_CLUSTER_TLOG")
_ALONE = [{}] + [{s: "1"} for s in SWITCHES] + [{"FHVAE_BIG_CELLS": "0"}, {"FHVAE_BIG_CELLS": "1"}]
#: every switch alone, and the same again under FHVAE_NO_CLUSTER=1 (there the cell rows stand on their own)
ENVS = _ALONE + [dict(e, FHVAE_NO_CLUSTER="1") for e in _ALONE[2:]]
ALL_VARS = SWITCHES + ("FHVAE_BIG_CELLS",)
QUERIES = ("fhvae_lstm_form", "fhvae_lstm_layout_id", "fhvae_lstm_pre_elems", "fhvae_lstm_ws_below_elems",
           "fhvae_lstm_infer_cs_elems")
_FAKE = 0x10000  # a non-NULL, 16-byte aligned address nobody reads


def env_name(env):
    return ",".join("%s=%s" % kv for kv in sorted(env.items())) or "none"


def cases():
    """(dtype, lp, H, L, B, T, (I, Ic)) in the order of the file's lists."""
    return list(itertools.product(DTYPES, LPS, HS, LS, BS, TS, IIC))


BLOCK = len(BS) * len(TS) * len(IIC)  # consecutive cases that share (dtype, lp, H, L)


def block_case(b):
    """(dtype, lp, H, L) of block b."""
    return cases()[b * BLOCK][:4]


def device_free(case, env):
    """The row does not depend on which device the library finds: no persistent form can be chosen."""
    return case[0] == 0 or not case[1] or "FHVAE_NO_CLUSTER" in env


def make_desc(hb, case):
    dtype, lp, H, L, B, T, (I, Ic) = case
    d = hb.LstmDesc()
    d.dtype, d.L, d.B, d.T, d.I, d.Ic, d.H = dtype, L, B, T, I, Ic, H
    for k in ("x", "xc", "hs", "cs", "gates", "pre"):
        setattr(d, k, _FAKE)
    for k in ("w_ih", "w_hh", "b_ih", "b_hh"):
        for l in range(L):
            getattr(d, k)[l] = _FAKE
    d.lp = _FAKE if lp else None
    return d


class set_env:
    """The schedule switches set to exactly `env` (the library reads them on every call), restored on exit."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in ALL_VARS}
        for k in ALL_VARS:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def sweep(lib, descs, env):
    """[(form, layout, pre, ws_below, infer_cs, lp_bytes)] of every descriptor under `env`."""
    fns = [getattr(lib, q) for q in QUERIES + ("fhvae_lstm_lp_bytes",)]
    with set_env(env):
        return [tuple(int(f(r)) for f in fns) for r in descs]


def digests(rows):
    """One digest per block of the rows of sweep()."""
    assert len(rows) % BLOCK == 0
    return [hashlib.sha256("\n".join(",".join(map(str, r)) for r in rows[b:b + BLOCK]).encode()).hexdigest()[:16]
            for b in range(0, len(rows), BLOCK)]


def census(rows):
    return dict(sorted(collections.Counter("form %d layout %d" % r[:2] for r in rows).items()))


def load():
    with open(GOLDEN) as f:
        return json.load(f)


def record(lib, hb):
    descs = [C.byref(make_desc(hb, c)) for c in cases()]
    rows = {env_name(e): sweep(lib, descs, e) for e in ENVS}
    return {"digests": {k: digests(r) for k, r in rows.items()}, "census": {k: census(r) for k, r in rows.items()}}


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "pytorch-scalablefhvae_amd"))
    import hip_binding as hb

    assert sys.argv[1:2] == ["--record"], __doc__
    out = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    gold = record(hb.load_library(), hb)
    assert {"form 1 layout 18", "form 2 layout 20"} <= set(gold["census"]["none"]), "no persistent form: not a MI355X?"
    with open(out, "w") as f:  # one line per switch setting
        f.write("{\n" + ",\n".join('"%s": {\n%s\n}' % (k, ",\n".join('"%s": %s' % (e, json.dumps(v)) for e, v in gold[k].items()))
                                  for k in ("digests", "census")) + "\n}\n")
    print("%d cases x %d switch settings -> %s" % (len(cases()), len(ENVS), out))
