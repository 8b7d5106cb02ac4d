"""One valid small call per MD_AOT_ARGS entry point of include/minddet_hip_pp.h, in the form of tests/abi_cases.py (operand kinds and rank
flags are explained there).  The feature's CPU test file hands each row to the single-defect test of tests/abi_derive.py, and
tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0."""
from tests.abi_cases import B16, F, I, U8, Case, S, T, i32   # noqa: F401

PPHead = S(("off_cls", i32), ("off_box", i32), ("off_dir", i32), ("num_anchors", i32), ("num_classes", i32), ("score_mode", i32),
           ("self_train", i32))


def _attrs():
    return PPHead(0, 4, 18, 2, 2, 0, 1)        # A = 2, K = 2: 4 class, 14 box and 4 direction channels of 24


def _cases():
    c = []
    # head [1, 2, 3, 24]: N = 2 x 3 x 2 = 12 anchors
    c.append(Case("md_pp_scores", [T((1, 2, 3, 24), B16), T((1, 12), U8, "opt"), T((1, 12), F), T((1, 12), I)], extra=_attrs(),
                  extra_required=True, tag="[mask]"))
    c.append(Case("md_pp_scores", [T((1, 2, 3, 24), B16), T((1, 12), U8, "opt", null=True), T((1, 12), F), T((1, 12), I)], extra=_attrs(),
                  extra_required=True, tag="[all]"))
    dec = [T((1, 2, 3, 24), B16), T((12, 7), F), T((1, 5), I), T((1,), I), T((1, 5), F), T((1, 12), I), T((1, 5, 9), F), T((1, 5, 4), F),
           T((1, 5), I)]
    c.append(Case("md_pp_decode_selected", dec + [T((1, 5, 7), F, "opt")], extra=_attrs(), extra_required=True, nparam={9, 10}, tag="[boxes]"))
    c.append(Case("md_pp_decode_selected", dec, extra=_attrs(), extra_required=True, nparam={9, 10}))
    return c


CASES = _cases()
