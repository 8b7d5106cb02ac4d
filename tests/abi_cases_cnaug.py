"""One valid small call per entry point of include/minddet_hip_cnaug.h (plus the optional-operand forms: colour NULL and given, workspace
and pool), in the form of tests/abi_cases.py (operand kinds and rank flags are explained there).  The feature's CPU test file hands each
row to the single-defect test of tests/abi_derive.py, and tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0."""
from tests.abi_cases import B16, F, I, U8, Case, S, T, f64, i32   # noqa: F401

F64 = "float64"
CNTransform = S(("rand_crop", i32), ("scale", f64), ("shift", f64), ("flip_prop", f64), ("in_h", i32), ("in_w", i32), ("down_ratio", i32))
CNImage = S(("out_h", i32), ("out_w", i32), ("pad_lo", i32), ("pad_hi", i32))


def transform_attrs(rand_crop=1):
    return CNTransform(rand_crop, 0.4, 0.1, 0.5, 24, 40, 4)


def _transform():
    # B = 2
    return [T((2, 2), I), T((2, 4), F64), T((2, 6), F), T((2, 6), F64), T((2,), I)]


def _image(colour, workspace, C=8, pad=(0, 0)):
    # B = 2, sources 8 x 12, output 6 x 10; the workspace: 8 B ((60 + 2047) / 2048 + 1) = 32 bytes
    lo, hi = pad
    ops = [T((2, 8, 12, 3), U8), T((2, 2), I), T((2, 6), F), T((6,), F), T((2, 8), F64, "opt", null=not colour),
           T((2, lo + 6 + hi, lo + 10 + hi, C), B16)]
    return ops + ([T((32,), U8, "opt", "free")] if workspace else [])


def _cases():
    return [Case("md_cn_aug_transform", _transform(), extra=transform_attrs(1), extra_required=True, tag="[rand_crop]"),
            Case("md_cn_aug_transform", _transform(), extra=transform_attrs(0), extra_required=True, tag="[scale, shift]"),
            Case("md_cn_aug_image", _image(True, True), extra=CNImage(6, 10, 0, 0), extra_required=True, nparam={6, 7}, tag="[colour, workspace]"),
            Case("md_cn_aug_image", _image(True, False, 4, (7, 9)), extra=CNImage(6, 10, 7, 9), extra_required=True, nparam={6, 7},
                 tag="[colour, pool, stem layout]"),
            Case("md_cn_aug_image", _image(False, False), extra=CNImage(6, 10, 0, 0), extra_required=True, nparam={6, 7}, tag="[no colour]")]


CASES = _cases()
