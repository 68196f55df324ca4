"""train_model.main feeds the model exactly what the commit that wrote tests/golden/train_trace.json fed it: every training and
dev forward (and every encode / encode_z2 of an estimate) with the same segments in the same order and batches against the same
number of table rows, the same exit code, the same printed text apart from the figures, the same files under --exp-dir and the
same checkpoint keys and shapes (tests/train_trace.py: what is recorded, the cases, and how the file is written)."""
import json

import pytest

import train_trace

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(train_trace.GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_every_case(golden):
    assert sorted(golden) == sorted(train_trace.CASES)


@pytest.mark.parametrize("name", sorted(train_trace.CASES))
def test_train_trace_matches_parent(golden, name):
    got = json.loads(json.dumps(train_trace.run_case(name)))  # (as the file holds it: keys as strings)
    diffs = train_trace.differences(got, golden[name], name)
    assert not diffs, "\n".join(diffs[:20])
