"""What the tools/bench_*.py measurement tools share: the import path of the package, median [min, max], the alternating
device-event loop, the "no GPU, no number" exit and the JSON-line sink.  Importing it puts the repository root and
pytorch-scalablefhvae_amd/ in front of sys.path."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-scalablefhvae_amd")]


def spread(ts):
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


def alternate(fns, reps, warmup=1):
    """{name: [ms]}: the functions in turn, `reps` rounds (an int, or {name: rounds} for a count per function), device events
    around every call."""
    import torch

    rounds = reps if isinstance(reps, dict) else dict.fromkeys(fns, reps)
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for r in range(max(rounds.values())):
        for name, fn in fns.items():
            if r >= rounds[name]:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1))
    return ts


def require_gpu(tool_name):
    import torch

    if not torch.cuda.is_available():
        sys.exit("%s measures on a MI355X: no GPU, no number" % tool_name)


def open_sink(path):
    """-> emit(res): prints res as one JSON line and, with a path, appends it to that file."""
    sink = open(path, "a") if path else None

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    return emit
