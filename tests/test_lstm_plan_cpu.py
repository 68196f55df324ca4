"""CPU twin of tests/test_lstm_plan_gpu.py: the blocks of tests/golden/lstm_plan.json that do not depend on the device (f32, `lp`
NULL, or FHVAE_NO_CLUSTER set: no persistent form can be chosen), against the same file."""
import ctypes as C

import pytest

import lstm_plan_sweep as S


@pytest.fixture(scope="module")
def swept():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding as hb

    cases = S.cases()
    return hb.load_library(), cases, [C.byref(S.make_desc(hb, c)) for c in cases], S.load()


@pytest.mark.parametrize("env", S.ENVS, ids=S.env_name)
def test_device_free_blocks_reproduce_the_recorded_table(swept, env):
    lib, cases, descs, gold = swept
    keep = [b for b in range(len(cases) // S.BLOCK) if S.device_free(cases[b * S.BLOCK], env)]
    assert len(keep) == (48 if "FHVAE_NO_CLUSTER" in env else 36)
    rows = S.sweep(lib, [d for b in keep for d in descs[b * S.BLOCK:(b + 1) * S.BLOCK]], env)
    want = gold["digests"][S.env_name(env)]
    bad = [S.block_case(b) for b, g in zip(keep, S.digests(rows)) if g != want[b]]
    assert not bad, "blocks (dtype, lp, H, L) that differ under %s: %r" % (S.env_name(env), bad)
    if len(keep) == 48:
        assert S.census(rows) == gold["census"][S.env_name(env)]


def test_golden_covers_every_edge():
    gold = S.load()
    assert list(gold["digests"]) == list(gold["census"]) == [S.env_name(e) for e in S.ENVS] and len(S.ENVS) == 18
    assert all(len(v) == 48 for v in gold["digests"].values()) and all(sum(v.values()) == 16800 for v in gold["census"].values())
    # rejected, step cells, large-tile cells, rows form, rows form with unit-major gates, contraction-split form
    assert set(gold["census"]["none"]) == {"form 0 layout -1", "form 0 layout 0", "form 0 layout 1", "form 1 layout 18",
                                           "form 1 layout 19", "form 2 layout 20"}
    assert "form 1 layout 19" not in gold["census"]["FHVAE_NO_RS=1"] and "form 1 layout 19" not in gold["census"]["FHVAE_NO_FWD_WR=1"]
    assert set(gold["census"]["FHVAE_NO_CLUSTER=1"]) == {"form 0 layout -1", "form 0 layout 0", "form 0 layout 1"}
