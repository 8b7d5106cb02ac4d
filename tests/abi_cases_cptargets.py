"""One valid small call of md_cp_assign_targets (include/minddet_hip_cptargets.h) per optional-operand form, in the form of
tests/abi_cases.py (operand kinds and rank flags are explained there).  The feature's CPU test file hands each row to the single-defect
test of tests/abi_derive.py, and tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0."""
from tests.abi_cases import F, I, U8, Case, S, T, f32, i32   # noqa: F401

CPTargets = S(("num_tasks", i32), ("num_classes", i32 * 8), ("voxel_size", f32 * 2), ("pc_range", f32 * 2), ("out_size_factor", i32),
              ("gaussian_overlap", f32), ("min_radius", i32))


def target_attrs():
    """T = 2 tasks of 1 and 2 classes on 0.8 m cells from (-3.2, -3.2)"""
    a = CPTargets()
    a.num_tasks = 2
    a.num_classes[0], a.num_classes[1] = 1, 2
    a.voxel_size[0] = a.voxel_size[1] = 0.2
    a.pc_range[0] = a.pc_range[1] = -3.2
    a.out_size_factor, a.gaussian_overlap, a.min_radius = 4, 0.1, 2
    return a


def _operands():
    # B = 1, G = 3, T = 2, C = 2, an 8 x 12 map (H = 8, W = 12), M = 4
    return [T((1, 3, 9), F), T((1, 3), I), T((1, 2, 2, 8, 12), F), T((1, 2, 4, 10), F), T((1, 2, 4), I), T((1, 2, 4), U8), T((1, 2, 4), I),
            T((1, 4, 10), F)]


def _cases():
    c = [Case("md_cp_assign_targets", _operands(), extra=target_attrs(), extra_required=True, nparam={8, 9}, tag="[pool]"),
         # the workspace given: B T (G + 1) x 16 = 128 bytes
         Case("md_cp_assign_targets", _operands() + [T((128,), U8, "opt", "free")], extra=target_attrs(), extra_required=True, nparam={8, 9},
              tag="[workspace]")]
    return c


CASES = _cases()
