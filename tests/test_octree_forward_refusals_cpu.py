"""The argument checks of the octree renderers answer as they did before the forward path was made one: for every row of
tests/golden/octree_forward_refusals.json (recorded by tests/_octree_forward_refusals.py on the commit before that change) the
return code and the whole pxo_last_error() text are equal.  The checks run before any HIP call: no GPU is needed."""
import json

import pytest

import _octree_forward_refusals as R
from plenoctree_amd import _lib

with open(R.GOLDEN) as _f:
    RECORDED = json.load(_f)
CASES = R.cases()


def test_the_recorded_rows_are_the_cases():
    assert sorted(RECORDED) == sorted(rid for rid, _, _ in CASES)
    assert {rid.split("/")[0] for rid in RECORDED} == set(R.ENTRIES)
    # only refusals and the no-work return are recorded: nothing here reaches a launch
    assert all(row["rc"] == -1 and row["error"] or (row["rc"], row["error"]) == (0, "") for row in RECORDED.values())


@pytest.mark.parametrize("rid,entry,spec", CASES, ids=[c[0] for c in CASES])
def test_return_code_and_message_are_unchanged(rid, entry, spec):
    rc, text = R.call(_lib, entry, spec)
    assert {"rc": rc, "error": text} == RECORDED[rid]
