"""One valid small call of md_cn_assign_targets, md_cn_loss and md_cn_loss_grad (include/minddet_hip_cn.h) per optional-operand form, in
the form of tests/abi_cases.py (operand kinds and rank flags are explained there).  The feature's CPU test file hands each row to the
single-defect test of tests/abi_derive.py, and tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0."""
from tests.abi_cases import B16, F, I, U8, Case, S, T, f32, i32

CNTargets = S(("min_overlap", f32))
CNLoss = S(("num_classes", i32), ("off_hm", i32), ("off_wh", i32), ("off_reg", i32), ("hm_weight", f32), ("wh_weight", f32),
           ("off_weight", f32))


def target_attrs():
    a = CNTargets()
    a.min_overlap = 0.7
    return a


def loss_attrs():
    """C = 3 classes: hm at 0, wh at 3, reg at 5 (Cp = 8)"""
    a = CNLoss()
    a.num_classes, a.off_hm, a.off_wh, a.off_reg = 3, 0, 3, 5
    a.hm_weight, a.wh_weight, a.off_weight = 1.0, 0.1, 1.0
    return a


def _target_operands():
    # B = 1, G = 3, C = 3, an 8 x 12 map (H = 8, W = 12), M = 4
    return [T((1, 3, 4), F), T((1, 3), I), T((1, 3, 8, 12), F), T((1, 4), I), T((1, 4), U8), T((1, 4, 2), F), T((1, 4, 2), F)]


def _loss_operands(grad):
    # B = 1, an 8 x 12 map, Cp = 8, C = 3, M = 4
    ops = [T((1, 8, 12, 8), B16), T((1, 3, 8, 12), F), T((1, 4), I), T((1, 4), U8), T((1, 4, 2), F), T((1, 4, 2), F), T((3,), F), T((1,), F),
           T((1,), F)]
    return ops + [T((1, 8, 12, 8), F)] if grad else ops


def _cases():
    c = [Case("md_cn_assign_targets", _target_operands(), extra=target_attrs(), extra_required=True, nparam={7, 8}, tag="[pool]"),
         # the workspace given: 16 B M = 64 bytes
         Case("md_cn_assign_targets", _target_operands() + [T((64,), U8, "opt", "free")], extra=target_attrs(), extra_required=True,
              nparam={7, 8}, tag="[workspace]")]
    for sym, grad, n in (("md_cn_loss", False, 9), ("md_cn_loss_grad", True, 10)):
        c.append(Case(sym, _loss_operands(grad), extra=loss_attrs(), extra_required=True, nparam={n, n + 1}, tag="[pool]"))
        # the workspace given: 8 B (4 + 2 ceil(H W / 64)) + 4 ceil(B C H W / 16384) = 8 x 8 + 4 = 68 bytes
        c.append(Case(sym, _loss_operands(grad) + [T((68,), U8, "opt", "free")], extra=loss_attrs(), extra_required=True, nparam={n, n + 1},
                      tag="[workspace]"))
    return c


CASES = _cases()
TARGET_CASES = [c for c in CASES if c.sym == "md_cn_assign_targets"]
LOSS_CASES = [c for c in CASES if c.sym != "md_cn_assign_targets"]
