"""One valid small call of md_pp_loss and md_pp_loss_grad (include/minddet_hip_pploss.h) per optional-operand form, in the form of
tests/abi_cases.py (operand kinds and rank flags are explained there).  The feature's CPU test file hands each row to the single-defect
test of tests/abi_derive.py, and tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0."""
from tests.abi_cases import B16, F, I, U8, Case, S, T, f32, i32

PPHead = S(*[(n, i32) for n in ("off_cls", "off_box", "off_dir", "num_anchors", "num_classes", "score_mode", "self_train")])
PPLoss = S(("head", PPHead), ("alpha", f32), ("gamma", f32), ("sigma", f32), ("code_weights", f32 * 7), ("cls_weight", f32),
           ("loc_weight", f32), ("dir_weight", f32), ("pos_cls_weight", f32), ("neg_cls_weight", f32))


def loss_attrs():
    """A = 2 anchors, K = 1 class, the three heads side by side from channel 0: cls 2, box 14, dir 4 (20 of C = 24 channels), the KITTI
    configurations' loss settings"""
    a = PPLoss()
    h = a.head
    h.off_cls, h.off_box, h.off_dir, h.num_anchors, h.num_classes, h.score_mode, h.self_train = 0, 2, 16, 2, 1, 0, 1
    a.alpha, a.gamma, a.sigma = 0.25, 2.0, 3.0
    for j in range(7):
        a.code_weights[j] = 1.0
    a.cls_weight, a.loc_weight, a.dir_weight, a.pos_cls_weight, a.neg_cls_weight = 1.0, 2.0, 0.2, 1.0, 1.0
    return a


def _operands(grad):
    # B = 1, an 8 x 12 map (H = 8, W = 12), C = 24, A = 2: N = 192
    ops = [T((1, 8, 12, 24), B16), T((1, 192), I), T((1, 192, 7), F), T((192, 7), F), T((5,), F), T((1,), F), T((1,), F)]
    return ops + [T((1, 8, 12, 24), F)] if grad else ops


def _cases():
    c = []
    for sym, grad, n in (("md_pp_loss", False, 7), ("md_pp_loss_grad", True, 8)):
        c.append(Case(sym, _operands(grad), extra=loss_attrs(), extra_required=True, nparam={n, n + 1}, tag="[pool]"))
        # the workspace given: 40 B ceil(H W / 64) + 4 B ceil(N / 4096) = 40 x 2 + 4 = 84 bytes
        c.append(Case(sym, _operands(grad) + [T((84,), U8, "opt", "free")], extra=loss_attrs(), extra_required=True, nparam={n, n + 1},
                      tag="[workspace]"))
    return c


CASES = _cases()
