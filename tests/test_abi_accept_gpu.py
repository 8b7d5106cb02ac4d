"""-m gpu: every valid row of every tests/abi_cases*.py table is ACCEPTED -- made exactly once through the C ABI with zero-filled tensors
(zero indices, counts and offsets are in range for every row), rc 0 each, one synchronise per table.  This is what makes the calls
tests/test_abi_checks_cpu.py derives from the same rows single-defect calls.  One pass: a call that is refused fails the test there."""
import pytest
import torch

from tests.abi_derive import all_rows
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
DT = {"float32": torch.float32, "float64": torch.float64, "bfloat16": torch.bfloat16, "int32": torch.int32, "int64": torch.int64,
      "uint8": torch.uint8}
ROWS = {"abi_cases": 54, "chain": 1, "cn": 6, "cnaug": 5, "cocoeval": 4, "convbwd": 11, "cp": 6, "cpaug": 8, "cploss": 4, "cpsweeps": 2,
        "cptargets": 2, "groupedbwd": 12, "kitti": 5, "kittieval": 9, "nusceval": 4, "pcaug": 5, "points": 3, "pp": 4, "pploss": 4,
        "ppreader": 4, "train": 10}


@pytest.mark.parametrize("table", ROWS)
def test_every_valid_row_is_accepted(table):
    from minddet_amd import _lib

    rows = all_rows()
    module = lambda t: t if t == "abi_cases" else "abi_cases_" + t
    assert {t for t, _ in rows} == {module(t) for t in ROWS}      # a new table gets its line above
    keep = []
    for case in (c for t, c in rows if t == module(table)):
        tensors = [None if t.null else torch.zeros(t.shape, dtype=DT[t.dtype], device=DEV) for t in case.operands]
        keep.append(tensors)    # alive until the one synchronise below
        assert _lib.call(case.sym, tensors, extra=case.extra) == 0, case.id     # (_lib.call raises MindDetHipError with the rc otherwise)
    torch.cuda.synchronize()
    assert len(keep) == ROWS[table]
