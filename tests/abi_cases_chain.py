"""One valid small call per MD_AOT_ARGS entry point of include/minddet_hip_chain.h, in the form of tests/abi_cases.py (operand kinds and
rank flags are explained there).  The feature's CPU test file hands each row to the single-defect test of tests/abi_derive.py, and
tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0."""
from tests.abi_cases import B16, F, Case, T


def _cases():
    # t2, res, w3, b3, w1, b1, y, t1 on a [1, 3, 5] image
    return [Case("md_pw_chain", [T((1, 3, 5, 128), B16), T((1, 3, 5, 512), B16), T((512, 128), B16), T((512,), F), T((128, 512), B16),
                                 T((128,), F), T((1, 3, 5, 512), B16), T((1, 3, 5, 128), B16)])]


CASES = _cases()
