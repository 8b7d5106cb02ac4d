"""One valid small call of md_cp_loss and md_cp_loss_grad (include/minddet_hip_cploss.h) per optional-operand form, in the form of
tests/abi_cases.py (operand kinds and rank flags are explained there).  The feature's CPU test file hands each row to the single-defect
test of tests/abi_derive.py, and tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0."""
from tests.abi_cases import B16, F, I, U8, Case, S, T, f32, i32

CPTask = S(*[(n, i32) for n in ("off_reg", "off_height", "off_dim", "off_rot", "off_vel", "off_hm", "num_classes", "class_base")])
CPLoss = S(("num_tasks", i32), ("task", CPTask * 8), ("weight", f32), ("code_weights", f32 * 10))


def loss_attrs():
    """T = 2 tasks of 1 and 2 classes, heads with vel side by side: 11 channels from 0, 12 from 11 (Cp = 24)"""
    a = CPLoss()
    a.num_tasks = 2
    base = 0
    for t, nc in enumerate((1, 2)):
        k = a.task[t]
        k.off_reg, k.off_height, k.off_dim, k.off_rot, k.off_vel, k.off_hm = base, base + 2, base + 3, base + 6, base + 8, base + 10
        k.num_classes = nc
        base += 10 + nc
    a.weight = 0.25
    for j, v in enumerate((1, 1, 1, 1, 1, 1, 0.2, 0.2, 1, 1)):
        a.code_weights[j] = v
    return a


def _operands(grad):
    # B = 1, an 8 x 12 map (H = 8, W = 12), Cp = 24, T = 2, C = 2, M = 4
    ops = [T((1, 8, 12, 24), B16), T((1, 2, 2, 8, 12), F), T((1, 2, 4, 10), F), T((1, 2, 4), I), T((1, 2, 4), U8), T((1, 2, 4), I),
           T((2, 12), F), T((2,), F), T((1,), F)]
    return ops + [T((1, 8, 12, 24), F)] if grad else ops


def _cases():
    c = []
    for sym, grad, n in (("md_cp_loss", False, 9), ("md_cp_loss_grad", True, 10)):
        c.append(Case(sym, _operands(grad), extra=loss_attrs(), extra_required=True, nparam={n, n + 1}, tag="[pool]"))
        # the workspace given: 8 B T (12 + ceil(H W / 64)) = 8 x 2 x 14 = 224 bytes
        c.append(Case(sym, _operands(grad) + [T((224,), U8, "opt", "free")], extra=loss_attrs(), extra_required=True, nparam={n, n + 1},
                      tag="[workspace]"))
    return c


CASES = _cases()
