"""One valid small call of include/minddet_hip_kittieval.h per call form, in the form of tests/abi_cases.py (operand kinds and rank flags
are explained there).  The feature's CPU test file hands each row to the single-defect test of tests/abi_derive.py, and
tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0.  The extents: I = 2 images, Gt = 5, Dt = 6, Cn = 2, K = 2, P
= 16 pairs."""
from tests.abi_cases import I64, U8, Case, I, S, T, i32

F64 = "float64"
NI, GT, DT, CN, K, P, PTS = 2, 5, 6, 2, 2, 16, 41
FlagsAttrs = S(("abs_gt_height", i32))
OverlapsAttrs = S(("metric", i32))
StatsAttrs = S(("metric", i32), ("compute_aos", i32))


def _match_operands():
    return [T((P,), F64), T((CN, 3, GT), U8), T((CN, 3, DT), U8), T((DT,), F64), T((NI + 1,), I), T((NI + 1,), I), T((NI + 1,), I64), T((CN, K), F64)]


def _overlaps(metric):
    w = 4 if metric == 0 else 7
    return Case("md_kitti_eval_overlaps", [T((NI + 1,), I), T((NI + 1,), I), T((NI + 1,), I64), T((GT, w), F64), T((DT, w), F64), T((P,), F64)],
                extra=OverlapsAttrs(metric), extra_required=True, tag=f"[metric {metric}]")


def _stats(metric, aos):
    ops = _match_operands() + [T((CN, 3, K, PTS), F64), T((CN, 3, K), I), T((GT, 4), F64), T((GT,), U8), T((DT, 4), F64), T((GT,), F64), T((DT,), F64),
                               T((CN, 3, K, PTS, NI, 3), I), T((CN, 3, K, PTS, NI), F64), T((CN, 3, K, PTS, 3), I), T((CN, 3, K, PTS), F64)]
    return Case("md_kitti_eval_stats", ops, extra=StatsAttrs(metric, aos), extra_required=True, tag=f"[metric {metric}, aos {aos}]")


def _cases():
    flags = [T((GT, 4), F64), T((GT,), I), T((GT,), F64), T((CN, GT), U8), T((DT, 4), F64), T((CN, DT), U8), T((CN, 3, GT), U8), T((CN, 3, DT), U8),
             T((CN, 3), I)]
    return [Case("md_kitti_eval_flags", flags, extra=FlagsAttrs(0), extra_required=True, tag="[full]"),
            Case("md_kitti_eval_flags", flags, extra=FlagsAttrs(1), extra_required=True, tag="[abs_gt_height]"),
            _overlaps(0), _overlaps(1), _overlaps(2),
            Case("md_kitti_eval_match", _match_operands() + [T((CN, 3, K, GT), F64)]),
            Case("md_kitti_eval_thresholds", [T((CN, 3, K, GT), F64), T((CN, 3), I), T((CN, 3, K, PTS), F64), T((CN, 3, K), I)]),
            _stats(0, 1), _stats(1, 0)]


CASES = _cases()
