"""One valid small call per entry point of include/minddet_hip_pcaug.h (plus the optional-operand forms), in the form of tests/abi_cases.py
(operand kinds and rank flags are explained there).  The feature's CPU test file hands each row to the single-defect test of
tests/abi_derive.py, and tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0."""
from tests.abi_cases import F, I, U8, Case, S, T, f32   # noqa: F401

F64 = "float64"
PCBoxes = S(("bv_range", f32 * 4))


def boxes_attrs():
    return PCBoxes((f32 * 4)(0.0, -39.68, 69.12, 39.68))


def _noise(grot):
    # B = 2, G = 3, T = 4
    return [T((2, 3, 7), F), T((2,), I), T((2, 3), U8), T((2, 3, 4, 3), F64), T((2, 3, 4), F64),
            T((2, 3, 4), F64, "opt", null=not grot), T((2, 3), I), T((2, 3, 4), F64), T((2, 3, 7), F)]


def _points(remove, workspace):
    # N = 300, B = 2, G = 3, R = 2; the workspace: 128 B (G + R) + 64 B + 4 (N / 256 + 3) = 1424 bytes with R = 2
    ops = [T((300, 4), F), T((3,), I), T((2, 3, 7), F), T((2,), I), T((2, 3), U8), T((2, 3, 4), F64),
           T((2, 2, 7), F, "opt", null=not remove), T((2,), I, "opt", null=not remove), T((2,), I, "opt", null=not remove),
           T((2, 6), F64), T((300, 4), F), T((3,), I), T((300,), I)]
    if workspace:
        ops.append(T((1424,), U8, "opt", "free"))
    return ops


def _cases():
    c = [Case("md_pc_noise_per_object", _noise(True), tag="[grot]"),
         Case("md_pc_noise_per_object", _noise(False), tag="[no grot]"),
         Case("md_pc_augment_points", _points(True, False), nparam={13, 14}, tag="[remove, pool]"),
         Case("md_pc_augment_points", _points(False, True), nparam={13, 14}, tag="[workspace]"),
         Case("md_pc_augment_boxes", [T((2, 3, 7), F), T((2,), I), T((2, 3), U8), T((2, 3), I), T((2, 6), F64), T((2, 3, 7), F), T((2, 3), I),
                                      T((2,), I)], extra=boxes_attrs(), extra_required=True)]
    return c


CASES = _cases()
