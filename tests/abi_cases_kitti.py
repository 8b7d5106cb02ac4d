"""One valid small call of include/minddet_hip_kitti.h per call form, in the form of tests/abi_cases.py (operand kinds and rank flags are
explained there).  The feature's CPU test file hands each row to the single-defect test of tests/abi_derive.py, and
tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0."""
from tests.abi_cases import F, I, U8, Case, S, T, f32, i32   # noqa: F401

F64 = "float64"
KittiRows = S(("limit_range", f32 * 6), ("use_limit", i32), ("lidar_input", i32))


def _crop(workspace):
    # N = 300, B = 2, K = 3; the workspace: 192 B K + 4 (N / 256 + 3) = 1168 bytes
    ops = [T((300, 4), F), T((3,), I), T((2, 3, 8, 3), F64), T((2,), I), T((300, 4), F), T((3,), I), T((300,), U8)]
    return ops + ([T((1168,), U8, "opt", "free")] if workspace else [])


def _rows(use_limit, lidar_input):
    at = KittiRows((f32 * 6)(0, -40, -5, 70, 40, 5), use_limit, lidar_input)
    ops = [T((2, 5, 9), F), T((2,), I), T((2, 4, 4), F64), T((2, 4, 4), F64), T((2, 2), I), T((2, 5, 14), F), T((2, 5), I), T((2,), I)]
    return Case("md_kitti_rows", ops, extra=at, extra_required=True, tag=f"[use_limit {use_limit}, lidar_input {lidar_input}]")


def _cases():
    return [Case("md_pc_crop_hulls", _crop(True), nparam={7, 8}, tag="[workspace]"),
            Case("md_pc_crop_hulls", _crop(False), nparam={7, 8}, tag="[pool]"),
            Case("md_kitti_boxes_to_lidar", [T((2, 5, 7), F), T((2,), I), T((2, 4, 4), F64), T((2, 5, 7), F)]),
            _rows(1, 0), _rows(0, 1)]


CASES = _cases()
