"""One valid small call of include/minddet_hip_cpsweeps.h per call form, in the form of tests/abi_cases.py (operand kinds and rank flags
are explained there).  The feature's CPU test file hands each row to the single-defect test of tests/abi_derive.py, and
tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0."""
from tests.abi_cases import F, I, U8, Case, S, T, f32, i32   # noqa: F401

F64 = "float64"
CPSweeps = S(("radius", f32), ("reserved0", i32))


def _merge(workspace, fin=5, m=300):
    # N = 300, B = 2, S = 3; the workspace: 4 (N / 256 + B S + 3) = 40 bytes
    ops = [T((300, fin), F), T((2, 3, 2), I), T((2, 3, 12), F64), T((2, 3), F64), T((2, 3), I), T((m, 5), F), T((3,), I), T((2,), I)]
    return ops + ([T((40,), U8, "opt", "free")] if workspace else [])


def _cases():
    return [Case("md_cp_sweeps_merge", _merge(True), extra=CPSweeps(1.0, 0), extra_required=True, nparam={8, 9}, tag="[workspace]"),
            Case("md_cp_sweeps_merge", _merge(False, fin=4, m=320), extra=CPSweeps(0.0, 0), extra_required=True, nparam={8, 9},
                 tag="[pool, 4-wide points, M > N]")]


CASES = _cases()
