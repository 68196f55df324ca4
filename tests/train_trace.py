"""Records what train_model.main feeds the model, case by case, for tests/test_train_trace_gpu.py.

What every training and dev forward receives depends only on seeds and integer bookkeeping (which segments, in which order, cut
into which batches, against how many table rows), never on kernel arithmetic: a refactor of the training loop must reproduce it
exactly.  `recording()` replaces `FHVAEBase.__call__` (the one method `model(...)` of both FHVAE and SimpleFHVAE goes through)
and the `encode` / `encode_z2` of both classes by wrappers that note, per call: model.training, num_seqs, whether mu2_table=
was passed, idx and nsegs as lists, the SHA-256 of the features' bytes and the batch size.  Per run of main(argv): the exit code,
stdout with every number replaced by `#` (and the run's temporary directory by `<tmp>`), the sorted file names under --exp-dir
and, for the last checkpoint, its keys, the shape of every tensor of its state_dict and epoch / best_epoch.

The golden file is produced by running this file as a script on the GPU (`python tests/train_trace.py --write`) and is only
ever regenerated from a train_model.py whose runs are known good: a refactor of the loop must pass against the file its parent
commit wrote.  `python tests/train_trace.py` compares a fresh run with the file and prints the fields that differ.
"""
import contextlib
import glob
import hashlib
import io
import json
import os
import re
import sys
import tempfile

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(_ROOT, "pytorch-scalablefhvae_amd"), _ROOT):  # (run as a script, or in a spawned rank: no conftest)
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(_ROOT, "tests", "golden", "train_trace.json")
NETS = ["--seg-len", "20", "--mels", "16", "--z1-hus", "16", "16", "--z2-hus", "16", "16", "--x-hus", "16", "16", "--z1-dim", "8",
        "--z2-dim", "8", "--epochs", "2"]
SYN = NETS + ["--train-segments", "37", "--dev-segments", "13", "--training-batch-size", "8", "--dev-batch-size", "8",
              "--num-seqs", "5"]
HS = ["--num-hierarchical-sequences", "2"]
_NUMBER = re.compile(r"-?\d+(?:\.\d+)?(?:[eE][-+]?\d+)?")


def _ints(v):
    return torch.as_tensor(v).reshape(-1).tolist()


def _sha(x):
    return hashlib.sha256(x.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


@contextlib.contextmanager
def recording(calls):
    import fhvae
    import fhvae_core
    import simple_fhvae

    call = torch.nn.Module.__call__

    def model_call(self, x, mu_idx, num_seqs, num_segs, **kw):
        calls.append(dict(fn="forward", training=bool(self.training), num_seqs=int(num_seqs), mu2_table=kw.get("mu2_table") is not None,
                          idx=_ints(mu_idx), nsegs=_ints(num_segs), x=_sha(x), batch=int(x.shape[0])))
        return call(self, x, mu_idx, num_seqs, num_segs, **kw)

    def encoder(name, fn):
        def wrapped(self, x):
            calls.append(dict(fn=name, training=bool(self.training), x=_sha(x), batch=int(x.shape[0])))
            return fn(self, x)
        return wrapped

    classes = (fhvae.FHVAE, simple_fhvae.SimpleFHVAE)
    kept = [(c, n, c.__dict__[n]) for c in classes for n in ("encode", "encode_z2")]
    fhvae_core.FHVAEBase.__call__ = model_call
    for c, n, fn in kept:
        setattr(c, n, encoder(n, fn))
    try:
        yield
    finally:
        del fhvae_core.FHVAEBase.__call__
        for c, n, fn in kept:
            setattr(c, n, fn)


def _checkpoint(exp):
    files = sorted(os.path.basename(p) for p in glob.glob(os.path.join(exp, "*")))
    runs = sorted((f for f in files if re.fullmatch(r"\w+_run_e\d+\.tar", f) and not f.startswith("best_model")),
                  key=lambda f: int(re.search(r"_e(\d+)\.tar", f).group(1)))
    ck = torch.load(os.path.join(exp, runs[-1]), map_location="cpu", weights_only=False)
    return dict(files=files, last=runs[-1], keys=sorted(ck), epoch=int(ck["epoch"]), best_epoch=int(ck["best_epoch"]),
                shapes={k: list(v.shape) for k, v in ck["state_dict"].items() if torch.is_tensor(v)})


def run_main(argv, tmp, exp=None):
    """One train_model.main(argv) under the recorder -> the run's record."""
    import train_model

    calls, buf = [], io.StringIO()
    with recording(calls), contextlib.redirect_stdout(buf):
        rc = train_model.main(list(argv))
    out = _NUMBER.sub("#", buf.getvalue().replace(str(tmp), "<tmp>"))
    rec = dict(rc=rc, stdout=out, calls=calls)
    if exp is not None:
        rec["exp"] = _checkpoint(exp)
    return rec


def corpus(tmp_path):
    """The numpy corpus that tests/test_hs_gpu.py trains on: the `corpus` fixture it imports from tests/test_data_ckpt_cpu.py."""
    rng = np.random.default_rng(0)
    lens = {"spk1_a": 57, "spk1_b": 20, "spk2_a": 19, "spk2_b": 133}
    with open(os.path.join(tmp_path, "feats.scp"), "w") as fs, open(os.path.join(tmp_path, "len.scp"), "w") as ls:
        for k, n in lens.items():
            feat = rng.normal(size=(n, 8)).astype(np.float32) * 3 + 1
            path = os.path.join(tmp_path, k + ".npy")
            np.save(path, feat)
            fs.write(f"{k} {path}\n")
            ls.write(f"{k} {n}\n")
    return tmp_path


def _rank(rank, world, port, argv_list, tmp, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    recs = []
    for i, argv in enumerate(argv_list):  # (one process group per main() call: main creates and destroys it)
        os.environ["MASTER_PORT"] = str(port + i)
        recs.append(run_main(argv, tmp))
    ret[rank] = recs


def two_ranks(argv_list, tmp, port):
    """[runs of rank 0, runs of rank 1]: two ranks sharing one GPU, as tests/test_dist_train_model_gpu.py."""
    import torch.multiprocessing as mp

    ret = mp.Manager().dict()
    mp.spawn(_rank, args=(2, port, argv_list, tmp, ret), nprocs=2, join=True)
    return [ret[0], ret[1]]


def _synthetic(extra):
    def case(tmp):
        return [run_main(SYN + extra, tmp)]
    return case


def _resume(tmp):
    exp = os.path.join(tmp, "exp")
    first = run_main(SYN + ["--exp-dir", exp], tmp, exp)
    again = run_main(SYN + ["--exp-dir", exp, "--continue-from", os.path.join(exp, "fhvae_run_e1.tar"), "--epochs", "3"], tmp, exp)
    return [first, again]


def _real(extra):
    def case(tmp):
        root = corpus(tmp)
        scp = ["--train-feat-scp", os.path.join(root, "feats.scp"), "--train-len-scp", os.path.join(root, "len.scp"),
               "--mvn-path", os.path.join(root, "mvn.json"), "--training-batch-size", "8", "--dev-batch-size", "8"]
        return [run_main(NETS + scp + extra, tmp)]
    return case


def _dist(extra, tag):
    def case(tmp):
        argv = SYN + ["--dist-backend", "gloo"] + extra
        return two_ranks([argv], tmp, 27100 + (os.getpid() % 100) * 4 + 450 * tag)
    return case


CASES = {
    "synthetic": _synthetic([]),                      # a ragged last batch in train (37 = 4 * 8 + 5) and dev (13 = 8 + 5)
    "synthetic_hs": _synthetic(HS),                   # 5 sequences in blocks of 2: a topped-up last block
    "synthetic_hierarchical": _synthetic(["--hierarchical"]),  # the estimate_mu2_dict initialisation
    "resume": _resume,                                # --exp-dir, then --continue-from its epoch-1 checkpoint with --epochs 3
    "real": _real([]),
    "real_hs": _real(HS),
    "two_ranks": _dist([], 0),                        # the last batch of 5 is cut to 4; one trace per rank
    "two_ranks_hs": _dist(HS, 1),
}


def run_case(name):
    with tempfile.TemporaryDirectory() as tmp:
        return CASES[name](tmp)


def differences(got, want, where=""):
    """The paths at which two records differ (empty: equal)."""
    if type(got) is not type(want):
        return ["%s: %r != %r" % (where, got, want)]
    if isinstance(got, dict):
        return [d for k in sorted(set(got) | set(want))
                for d in (differences(got[k], want[k], "%s.%s" % (where, k)) if k in got and k in want
                          else ["%s.%s: only in %s" % (where, k, "this run" if k in got else "the golden file")])]
    if isinstance(got, list):
        if len(got) != len(want):
            return ["%s: %d entries != %d" % (where, len(got), len(want))]
        return [d for i, (g, w) in enumerate(zip(got, want)) for d in differences(g, w, "%s[%d]" % (where, i))]
    return [] if got == want else ["%s: %r != %r" % (where, got, want)]


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    traces = {name: run_case(name) for name in CASES}
    if "--write" in argv:
        os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
        with open(GOLDEN, "w") as f:
            f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(traces[k], sort_keys=True)) for k in sorted(traces))
                    + "\n}\n")  # (one case per line)
        print("wrote %s: %d cases" % (GOLDEN, len(traces)))
        return 0
    with open(GOLDEN) as f:
        want = json.load(f)
    diffs = differences(json.loads(json.dumps(traces)), want)
    print("\n".join(diffs[:50]) if diffs else "identical: %d cases" % len(traces))
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
