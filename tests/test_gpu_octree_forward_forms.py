"""The forward renderers of the float, float16 and palette trees return the bits they returned before their host path was
made one: SHA-256 of every output against tests/golden/octree_forward_forms.json (recorded by tests/_octree_forward_forms.py
on the commit before that change, on an MI355X), and the float16 tree hash for hash the float tree."""
import json

import pytest
import torch

import _octree_forward_forms as F

pytestmark = pytest.mark.gpu

with open(F.GOLDEN) as _f:
    RECORDED = json.load(_f)
CASES = sorted({k.split("/lanes")[0] for k in RECORDED})


@pytest.fixture(scope="module")
def measured():
    from plenoctree_amd import octree_ops as oops
    return F.measure(oops, torch.device("cuda:0"))          # restores the lane override in a finally


def test_the_recorded_keys_are_the_cases(measured):
    assert sorted(measured) == sorted(RECORDED)
    want = [f"{form}/{kind}{K}" for form in ("float", "half") for kind, K in F.TREE_CASES]
    want += [f"quant/{what}_K{K}_r{r}_b{b}" for what in ("plain", "aux") for K, r, b in F.QUANT_CASES]
    assert CASES == sorted(want)
    assert len(RECORDED) == len(want) * len(F.LANES) * 2 * 2


@pytest.mark.parametrize("case", CASES)
def test_every_hash_equals_the_recorded_one(measured, case):
    keys = [k for k in RECORDED if k.split("/lanes")[0] == case]
    assert len(keys) == len(F.LANES) * 2 * 2
    assert {k: measured[k] for k in keys} == {k: RECORDED[k] for k in keys}


@pytest.mark.parametrize("kind,K", F.TREE_CASES)
def test_half_equals_float_hash_for_hash(measured, kind, K):
    floats = {k[len("float/"):]: v for k, v in measured.items() if k.startswith(f"float/{kind}{K}/")}
    halves = {k[len("half/"):]: v for k, v in measured.items() if k.startswith(f"half/{kind}{K}/")}
    assert len(floats) == len(F.LANES) * 2 * 2 and floats == halves
