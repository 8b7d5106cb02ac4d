"""One valid small call of include/minddet_hip_nusceval.h per call form, in the form of tests/abi_cases.py (operand kinds and rank flags
are explained there).  The feature's CPU test file hands each row to the single-defect test of tests/abi_derive.py, and
tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0.  The extents: I = 2 samples, Kc = 3 classes (C = 6 cells), Gt
= 5, Dt = 8 = I max_det with max_det = 4, D = 4, R = 101, L = 3 labels."""
from tests.abi_cases import F, Case, I, S, T, i32

F64 = "float64"
NI, KC, CELLS, GT, MAX_DET, DT, ND, NR, NL = 2, 3, 6, 5, 4, 8, 4, 101, 3
RowsAttrs = S(("first_sample", i32))
EvalAttrs = S(("tp_index", i32))


def _rows(batch, first, tag):
    ops = [T((batch, MAX_DET, 11), F), T((batch,), I), T((batch, 14), F64), T((NL,), I), T((KC,), F64), T((KC,), I), T((KC,), I),
           T((DT, 3), F64), T((DT, 3), F64), T((DT, 4), F64), T((DT, 2), F64), T((DT,), F64), T((DT,), F64), T((DT,), I), T((DT,), I), T((DT,), I),
           T((DT,), I), T((CELLS,), I), T((CELLS,), I)]
    return Case("md_nusc_rows", ops, extra=RowsAttrs(first), extra_required=True, tag=tag)


def _cases():
    match = [T((CELLS,), I), T((CELLS,), I), T((CELLS,), I), T((CELLS,), I), T((GT, 2), F64), T((GT, 3), F64), T((GT,), F64), T((GT, 2), F64), T((GT,), I),
             T((DT, 3), F64), T((DT, 3), F64), T((DT,), F64), T((DT, 2), F64), T((DT,), I), T((ND,), F64), T((KC,), F64),
             T((ND, DT), I), T((DT, 5), F64), T((CELLS,), I)]
    accum = [T((DT,), I), T((KC + 1,), I), T((DT,), F64), T((ND, DT), I), T((DT, 5), F64), T((CELLS,), I), T((NR,), F64),
             T((KC, ND, NR), F64), T((KC, ND, NR), F64), T((KC, 5, NR), F64), T((KC,), I), T((KC, ND), I), T((ND, DT), I), T((DT,), F64), T((5, DT), F64)]
    return [_rows(NI, 0, "[whole set]"), _rows(1, 1, "[second sample]"), Case("md_nusc_eval_match", match, extra=EvalAttrs(2), extra_required=True),
            Case("md_nusc_eval_accumulate", accum, extra=EvalAttrs(2), extra_required=True)]


CASES = _cases()
