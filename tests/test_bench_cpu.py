"""bench.py's protection of the first multi-GPU run (no GPU needed): the watchdog that prints what was already measured when a
phase does not come back, and the self-launcher's time limit with one fresh retry; --dump-outputs' writer; what a plain and a
--full run measure beside the headline."""
import os
import subprocess
import sys
import textwrap
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(code, env=None, timeout=120):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([sys.executable, "-c", textwrap.dedent(code)], cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)


def test_watchdog_emits_the_prepared_record_and_ends_the_process():
    r = _run("""
        import sys, time
        sys.path.insert(0, ".")
        import bench
        bench.WATCHDOG["emit"] = lambda what: print("RECORD after [%s]" % what, flush=True)
        bench.watchdog_arm(1, "captured replay")
        time.sleep(30)          # the "hung" main thread
        print("not reached")
    """)
    assert r.returncode == 0, r.stderr
    assert "RECORD after [captured replay]" in r.stdout and "not reached" not in r.stdout
    assert "did not finish in time" in r.stderr


def test_watchdog_disarmed_or_without_a_record():
    r = _run("""
        import sys, time
        sys.path.insert(0, ".")
        import bench
        bench.WATCHDOG["emit"] = lambda what: print("RECORD")
        bench.watchdog_arm(1, "phase")
        bench.watchdog_disarm()
        time.sleep(2.5)
        print("finished normally")
    """)
    assert r.returncode == 0 and "finished normally" in r.stdout and "RECORD" not in r.stdout
    r = _run("""
        import sys, time
        sys.path.insert(0, ".")
        import bench
        bench.watchdog_arm(1, "nothing measured yet")
        time.sleep(30)
    """)
    assert r.returncode == 3   # nothing to report: a failure, not a fake record


def test_self_launch_kills_a_stuck_rank_tree_and_retries_once():
    t0 = time.time()
    r = _run("""
        import sys, types
        sys.path.insert(0, ".")
        import bench
        args = types.SimpleNamespace(gpus=2, launch_timeout=4)
        print("rc", bench.self_launch(args, ["--gpus", "2"]))
    """, env={"FHVAE_BENCH_TEST_SLEEP": "600"}, timeout=300)
    assert "rc 124" in r.stdout, (r.stdout, r.stderr[-2000:])
    assert "starting a fresh one with --no-dist-graph --no-alt" in r.stderr and "second attempt did not finish either" in r.stderr
    assert time.time() - t0 < 200


def test_dump_outputs_types_budget_and_fixed_sample(tmp_path):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench

    g = torch.Generator().manual_seed(0)
    arrays = {"loss": torch.tensor(3.5, dtype=torch.float64), "small": torch.randn(7, 5, generator=g).bfloat16(),
              "big": torch.randn(1000, 64, generator=g), "bigger": torch.randn(4000, 32, generator=g)}
    limit = 700_000
    what = bench.dump_outputs(str(tmp_path / "a"), arrays, limit=limit)
    files = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in arrays}
    assert sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in arrays) <= limit
    assert files["loss"].dtype == np.float64 and files["loss"] == 3.5
    assert files["small"].dtype == np.float32 and np.array_equal(files["small"], arrays["small"].float().numpy())
    assert what["loss"] == what["small"] == what["big"] == "whole"
    np.testing.assert_array_equal(files["big"], arrays["big"].numpy())
    assert what["bigger"].startswith("sample ") and files["bigger"].dtype == np.float32
    assert np.isin(files["bigger"], arrays["bigger"].numpy()).all()
    # the same arrays give the same sample
    bench.dump_outputs(str(tmp_path / "b"), arrays, limit=limit)
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "bigger.npy"), files["bigger"])


def test_plain_run_measures_the_headline_alone_and_full_everything_else():
    sys.path.insert(0, ROOT)
    import bench

    def want(argv, world=1, use_dist=False):
        return bench.extras(bench.parse_args(argv), world, use_dist)

    base = ["--gpus", "1", "--steps", "5", "--warmup", "2"]
    for extra in ([], ["--config", "c4"], ["--idx", "zipf"], ["--dump-outputs", "d"], ["--batch", "256"]):
        assert want(base + extra) == set()
    assert want(["--gpus", "2"], world=2, use_dist=True) == set()
    assert want(["--force-dist"], use_dist=True) == set()
    # --full: each extra where the workload has it, unless its --no-* option is given
    assert want(base + ["--full"]) == {"roofline", "hbm", "alt", "cpu_baseline"}
    assert want(base + ["--full", "--no-roofline"]) == {"alt", "cpu_baseline"}
    assert want(base + ["--full", "--no-hbm", "--no-alt", "--no-cpu-baseline"]) == {"roofline"}
    assert want(base + ["--full", "--config", "c4"]) == {"roofline", "cpu_baseline"}
    assert want(base + ["--full", "--batch", "256"]) == {"roofline", "hbm", "cpu_baseline"}
    assert want(["--full", "--force-dist"], use_dist=True) == {"roofline", "hbm", "cpu_baseline"}
    assert want(["--gpus", "2", "--full"], world=2, use_dist=True) == {"roofline", "alt"}
