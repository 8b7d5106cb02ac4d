"""One valid small call of md_conv1x1_bwd_weight, md_grad_sumsq and md_adam_step (include/minddet_hip_train.h) per optional-operand form,
in the form of tests/abi_cases.py (operand kinds and rank flags are explained there).  The feature's CPU test file hands each row to the
single-defect test of tests/abi_derive.py, and tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0."""
from tests.abi_cases import B16, F, U8, Case, S, T, f64, i32

F64 = "float64"
Conv1x1Bwd = S(*[(n, i32) for n in ("cin", "cout", "x_c_off", "dy_c_off", "reserved0")])
AdamAttrs = S(*[(n, f64) for n in ("lr", "beta1", "beta2", "beta1_power", "beta2_power", "eps", "weight_decay", "max_norm", "grad_scale",
                                   "reserved0")])


def conv_attrs():
    """cin 8 of the 16 channels of x from channel 8 on, cout 3 of the 8 channels of dy from channel 2 on"""
    return Conv1x1Bwd(8, 3, 8, 2, 0)


def adam_attrs(max_norm=0.0):
    return AdamAttrs(1e-3, 0.9, 0.999, 0.9, 0.999, 1e-8, 1e-4, max_norm, 1.0, 0.0)


def _conv_operands(db):
    # N = 1, a 3 x 5 map: P = 15 pixels; dw [32, 64] is the pack of an 8 -> 3 layer, db its bias
    return [T((1, 3, 5, 16), B16), T((1, 3, 5, 8), F), T((32, 64), F), T((32,), F, "opt", null=not db)]


def _cases():
    c = []
    for db in (True, False):
        tag = "" if db else ", no db"
        c.append(Case("md_conv1x1_bwd_weight", _conv_operands(db), extra=conv_attrs(), extra_required=True, nparam={4, 5}, tag=f"[pool{tag}]"))
        # the workspace given: one slab of R = 16 rows of cin + 1 floats = 4 x 16 x 9 = 576 bytes
        c.append(Case("md_conv1x1_bwd_weight", _conv_operands(db) + [T((576,), U8, "opt", "free")], extra=conv_attrs(), extra_required=True,
                      nparam={4, 5}, tag=f"[workspace{tag}]"))
    c.append(Case("md_grad_sumsq", [T((100,), F), T((1,), F64)], nparam={2, 3}, tag="[pool]"))
    c.append(Case("md_grad_sumsq", [T((100,), F), T((1,), F64), T((8,), U8, "opt", "free")], nparam={2, 3}, tag="[workspace]"))   # one partial
    for clip in (True, False):
        for shadow in (True, False):
            ops = [T((100,), F), T((2,), F64, "opt", null=not clip), T((100,), F), T((100,), F), T((100,), F), T((60,), B16, "opt", null=not shadow)]
            c.append(Case("md_adam_step", ops, extra=adam_attrs(35.0 if clip else 0.0), extra_required=True,
                          tag=f"[{'sumsq' if clip else 'no sumsq'}, {'shadow' if shadow else 'no shadow'}]"))
    return c


CASES = _cases()
