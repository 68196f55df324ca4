"""The six LSTM schedule queries over the sweep of tests/lstm_plan_sweep.py reproduce tests/golden/lstm_plan.json, recorded on a
MI355X from the library as it was before one plan (csrc/lstm_cluster.h, LstmPlan) decided the schedule.  No kernel is launched:
the GPU is needed only because the persistent forms are chosen when the device check passes."""
import ctypes as C

import pytest

import lstm_plan_sweep as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def swept():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding as hb

    return hb.load_library(), [C.byref(S.make_desc(hb, c)) for c in S.cases()], S.load()


@pytest.mark.parametrize("env", S.ENVS, ids=S.env_name)
def test_queries_reproduce_the_recorded_table(swept, env):
    lib, descs, gold = swept
    rows = S.sweep(lib, descs, env)
    assert len(rows) == 16800
    got, want = S.digests(rows), gold["digests"][S.env_name(env)]
    bad = [S.block_case(b) for b in range(len(want)) if got[b] != want[b]]
    assert len(got) == len(want) and not bad, "blocks (dtype, lp, H, L) that differ under %s: %r" % (S.env_name(env), bad)
    assert S.census(rows) == gold["census"][S.env_name(env)]
    if "FHVAE_NO_CLUSTER" not in env:  # the device check passed: both persistent forms are in the table
        assert {1, 2} <= {r[0] for r in rows}
