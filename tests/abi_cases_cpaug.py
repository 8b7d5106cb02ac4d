"""One valid small call per entry point of include/minddet_hip_cpaug.h (plus the optional-operand forms), in the form of tests/abi_cases.py
(operand kinds and rank flags are explained there).  The feature's CPU test file hands each row to the single-defect test of
tests/abi_derive.py, and tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0."""
from tests.abi_cases import F, I, U8, Case, S, T, f32, i32   # noqa: F401

F64 = "float64"
CPCount = S(("min_points", i32))
CPBoxes = S(("bv_range", f32 * 4))


def boxes_attrs():
    return CPBoxes((f32 * 4)(-51.2, -51.2, 51.2, 51.2))


def _count(workspace):
    # N = 300, B = 2, G = 3; the workspace: 96 B G = 576 bytes
    ops = [T((300, 5), F), T((3,), I), T((2, 3, 9), F), T((2,), I), T((2, 3), I), T((2, 3), U8)]
    return ops + ([T((576,), U8, "opt", "free")] if workspace else [])


def _select(workspace):
    # B = 2, G = 3, S = 4; the workspace: 8 B S ((G + S + 63) / 64) = 64 bytes
    ops = [T((2, 3, 9), F), T((2,), I), T((2, 3), U8), T((2, 4, 9), F), T((2,), I), T((2, 4), I), T((2, 4), U8)]
    return ops + ([T((64,), U8, "opt", "free")] if workspace else [])


def _points(cand, workspace):
    # N = 300, Ns = 40, B = 2, S = 4; the workspace: 64 B + (N + Ns) + 4 ((N + Ns) / 256 + 3) = 484 bytes with the candidates
    ns = 40 if cand else 0
    ops = [T((300, 5), F), T((3,), I), T((40, 5), F, "opt", null=not cand), T((9,), I, "opt", null=not cand),
           T((2, 4, 9), F, "opt", null=not cand), T((2, 4), U8, "opt", null=not cand), T((2, 7), F64), T((300 + ns, 5), F), T((3,), I)]
    return ops + ([T((484,), U8, "opt", "free")] if workspace else [])


def _boxes(cand):
    s = 4 if cand else 0
    return [T((2, 3, 9), F), T((2, 3), I), T((2,), I), T((2, 3), U8), T((2, 4, 9), F, "opt", null=not cand), T((2, 4), I, "opt", null=not cand),
            T((2, 4), U8, "opt", null=not cand), T((2, 7), F64), T((2, 3 + s, 9), F), T((2, 3 + s), I), T((2,), I)]


def _cases():
    return [Case("md_cp_aug_count_points", _count(True), extra=CPCount(5), extra_required=True, nparam={6, 7}, tag="[workspace]"),
            Case("md_cp_aug_count_points", _count(False), extra=CPCount(-1), extra_required=True, nparam={6, 7}, tag="[pool]"),
            Case("md_cp_aug_select", _select(True), nparam={7, 8}, tag="[workspace]"),
            Case("md_cp_aug_select", _select(False), nparam={7, 8}, tag="[pool]"),
            Case("md_cp_aug_points", _points(True, True), nparam={9, 10}, tag="[candidates, workspace]"),
            Case("md_cp_aug_points", _points(False, False), nparam={9, 10}, tag="[no candidates, pool]"),
            Case("md_cp_aug_boxes", _boxes(True), extra=boxes_attrs(), extra_required=True, tag="[candidates]"),
            Case("md_cp_aug_boxes", _boxes(False), extra=boxes_attrs(), extra_required=True, tag="[no candidates]")]


CASES = _cases()
