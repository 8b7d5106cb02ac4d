"""One valid small call per MD_AOT_ARGS entry point of include/minddet_hip_cp.h and per optional-operand form, in the form of
tests/abi_cases.py (operand kinds and rank flags are explained there).  The feature's CPU test file hands each row to the single-defect
test of tests/abi_derive.py, and tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0."""
from tests.abi_cases import B16, F, I, Case, S, T, f32, i32   # noqa: F401

MAX_TASKS = 8
NmsRotated = S(("iou_threshold", f32), ("mode", i32), ("max_output", i32))
CPTask = S(("off_reg", i32), ("off_height", i32), ("off_dim", i32), ("off_rot", i32), ("off_vel", i32), ("off_hm", i32), ("num_classes", i32),
           ("class_base", i32))
CPHead = S(("num_tasks", i32), ("task", CPTask * MAX_TASKS), ("score_threshold", f32), ("out_size_factor", f32), ("voxel_size", f32 * 2),
           ("pc_range", f32 * 2), ("post_center_range", f32 * 6), ("max_per_task", i32))


def head_attrs():
    """T = 2 tasks in 24 channels: task 0 with a vel head and one class (channels 0 .. 10), task 1 without and two classes (11 .. 20);
    max_per_task 2"""
    a = CPHead()
    a.num_tasks = 2
    a.task[0] = CPTask(0, 2, 3, 6, 8, 10, 1, 0)
    a.task[1] = CPTask(11, 13, 14, 17, -1, 19, 2, 1)
    a.score_threshold, a.out_size_factor = 0.1, 4.0
    a.voxel_size[0] = a.voxel_size[1] = 0.2
    a.pc_range[0] = a.pc_range[1] = -1.6
    for i, v in enumerate((-5.0, -5.0, -10.0, 5.0, 5.0, 10.0)):
        a.post_center_range[i] = v
    a.max_per_task = 2
    return a


def _cases():
    c = []
    nms = NmsRotated(0.5, 0, 0)
    c.append(Case("md_nms_rotated", [T((2, 4, 7), F), T((2,), I, "opt"), T((2, 4), I), T((2,), I)], extra=nms, extra_required=True,
                  nparam={4, 5}, tag="[count]"))
    c.append(Case("md_nms_rotated", [T((2, 4, 7), F), T((2,), I, "opt", null=True), T((2, 4), I), T((2,), I)], extra=NmsRotated(0.5, 1, 3),
                  extra_required=True, nparam={4, 5}, tag="[all]"))
    c.append(Case("md_nms_rotated", [T((4, 7), F), T((1,), I, "opt"), T((4,), I), T((1,), I)], extra=nms, extra_required=True, nparam={4, 5},
                  tag="[one list]"))
    # head [1, 4, 4, 24]: n = 16 cells, T = 2, k = 3, m = 2
    c.append(Case("md_cp_scores", [T((1, 4, 4, 24), B16), T((1, 2, 16), F)], extra=head_attrs(), extra_required=True))
    c.append(Case("md_cp_decode_selected", [T((1, 4, 4, 24), B16), T((1, 2, 3), I), T((1, 2), I), T((1, 2, 3, 9), F), T((1, 2, 3, 7), F),
                                            T((1, 2, 3), I)], extra=head_attrs(), extra_required=True))
    c.append(Case("md_cp_pack", [T((1, 2, 3, 9), F), T((1, 2, 3), F), T((1, 2, 3), I), T((1, 2, 3), I), T((1, 2), I), T((1, 2), I), T((1, 4, 11), F),
                                 T((1,), I)], extra=head_attrs(), extra_required=True))
    return c


CASES = _cases()
