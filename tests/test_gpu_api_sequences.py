"""The render and train sequences of pxo_api.hip against numbers recorded from the commit before they were unified
(tests/golden/api_sequences.json, written by tests/_api_sequences.py on that commit's build): every workspace size, the launches
and rows each sequence puts under every profiler tag, dense, NeRF-SG and culled, and the bits a culled render and a culled step
leave when they share one workspace (arrays of the cull block that moved onto one another would change them).  What the sequences
compute is held by tests/test_gpu_parity.py, test_gpu_occupancy.py, test_gpu_occ_train.py and test_gpu_sg_train.py."""
import json

import pytest
import torch

import _api_sequences as A
from _helpers import _gpu, _ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(A.GOLDEN) as f:
        want = json.load(f)
    cus = torch.cuda.get_device_properties(_gpu()).multi_processor_count
    if cus != want["cus"]:                                        # the weight-gradient slabs, and so the sizes, follow the CU count
        pytest.skip(f"api_sequences.json was recorded on a device with {want['cus']} CUs, this one has {cus}")
    return want


def test_the_golden_file_holds_every_configuration(golden):
    assert sorted(golden["configs"]) == sorted(A.key(*c) for c in A.configs())
    for rec in golden["configs"].values():
        assert sorted(rec) == [f"precision{p}" for p in A.PRECISIONS]


@pytest.mark.parametrize("cfg", A.configs(), ids=lambda c: A.key(*c))
def test_sequences_equal_the_recorded_ones(golden, cfg):
    got = json.loads(json.dumps(A.measure_one(_ops(), _gpu(), *cfg)))              # tuples -> lists, as in the file
    want = golden["configs"][A.key(*cfg)]
    for precision, rec in want.items():
        for part in ("workspace_bytes", "launches", "shared_workspace"):
            for name, value in rec[part].items():
                print(precision, part, name, got[precision][part][name], value)
                assert got[precision][part][name] == value, (precision, part, name)
        assert got[precision] == rec
