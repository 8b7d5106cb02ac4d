"""-m gpu: every valid row of tests/abi_cases.py is ACCEPTED -- made exactly once through the C ABI with zero-filled tensors (zero
indices, counts and offsets are in range for every row), rc 0 each, one synchronise at the end.  This is what makes the calls
tests/test_abi_checks_cpu.py derives from the same rows single-defect calls.  One pass: a call that is refused fails the test there."""
import pytest
import torch

from tests.abi_cases import CASES
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
DT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "int32": torch.int32, "int64": torch.int64, "uint8": torch.uint8}


def test_every_valid_row_is_accepted():
    from minddet_amd import _lib

    keep = []
    for case in CASES:
        tensors = [None if t.null else torch.zeros(t.shape, dtype=DT[t.dtype], device=DEV) for t in case.operands]
        keep.append(tensors)    # alive until the one synchronise below
        assert _lib.call(case.sym, tensors, extra=case.extra) == 0, case.id     # (_lib.call raises MindDetHipError with the rc otherwise)
    torch.cuda.synchronize()
