"""One valid small call of include/minddet_hip_cocoeval.h per call form, in the form of tests/abi_cases.py (operand kinds and rank flags
are explained there).  The feature's CPU test file hands each row to the single-defect test of tests/abi_derive.py, and
tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0.  The extents: I = 2 images, Kc = 3 categories (C = 6 cells),
Gt = 5, Dt = 8 = I max_det with max_det = 4, T = 10, R = 101, A = 4, M = 3, L = 3 labels."""
from tests.abi_cases import F, U8, Case, I, S, T, i32

F64 = "float64"
NI, KC, CELLS, GT, MAX_DET, DT, NT, NR, NA, NM, NL = 2, 3, 6, 5, 4, 8, 10, 101, 4, 3, 3
RowsAttrs = S(("first_image", i32))


def _rows(batch, first, tag):
    ops = [T((batch, MAX_DET, 6), F), T((batch,), I), T((NL,), I), T((DT, 4), F64), T((DT,), F64), T((DT,), F64), T((DT,), I), T((DT,), I),
           T((CELLS,), I), T((CELLS,), I), T((DT,), I)]
    return Case("md_coco_eval_rows", ops, extra=RowsAttrs(first), extra_required=True, tag=tag)


def _cases():
    match = [T((CELLS,), I), T((CELLS,), I), T((CELLS,), I), T((CELLS,), I), T((GT, 4), F64), T((GT,), F64), T((GT,), U8), T((GT,), U8), T((DT, 4), F64),
             T((DT,), F64), T((NT,), F64), T((NA, 2), F64), T((NA, NT, DT), I), T((NA, NT, DT), U8), T((NA, CELLS), I)]
    accum = [T((DT,), I), T((KC + 1,), I), T((DT,), I), T((NA, NT, DT), I), T((NA, NT, DT), U8), T((NA, CELLS), I), T((NR,), F64), T((NM,), I),
             T((NT, NR, KC, NA, NM), F64), T((NT, KC, NA, NM), F64), T((NA, KC), I)]
    return [_rows(NI, 0, "[whole set]"), _rows(1, 1, "[second image]"), Case("md_coco_eval_match", match), Case("md_coco_eval_accumulate", accum)]


CASES = _cases()
