"""One valid small call per MD_AOT_ARGS entry point of include/minddet_hip_ppreader.h, in the form of tests/abi_cases.py (operand kinds and
rank flags are explained there).  The feature's CPU test file hands each row to the single-defect test of tests/abi_derive.py, and
tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0."""
from tests.abi_cases import B16, F, I, U8, Case, S, T, f32, i32   # noqa: F401

PPPillarEncode = S(("vx", f32), ("vy", f32), ("vz", f32), ("x_offset", f32), ("y_offset", f32), ("z_offset", f32), ("with_distance", i32),
                   ("reserved0", i32))
AnchorMask = S(("grid_x", i32), ("grid_y", i32), ("voxel_x", f32), ("voxel_y", f32), ("offset_x", f32), ("offset_y", f32),
               ("area_threshold", f32))


def _cases():
    c = []
    ops = [T((2, 8, 6, 4), F), T((2, 8), I), T((2, 8, 4), I), T((2,), I)]
    tail = [T((64,), F), T((64,), F), T((2, 16, 16, 64), B16)]
    c.append(Case("md_pp_pillar_encode", ops + [T((64, 10), F)] + tail, extra=PPPillarEncode(0.16, 0.16, 4.0, 0.08, -1.2, -1.0, 0, 0),
                  extra_required=True, tag="[k10]"))
    c.append(Case("md_pp_pillar_encode", ops + [T((64, 11), F)] + tail, extra=PPPillarEncode(0.16, 0.16, 4.0, 0.08, -1.2, -1.0, 1, 0),
                  extra_required=True, tag="[k11]"))
    am = AnchorMask(8, 8, 0.16, 0.16, 0.0, 0.0, 1.0)
    mask = [T((2, 8, 4), I), T((2,), I), T((5, 4), F), T((2, 5), U8)]
    c.append(Case("md_pp_anchor_mask", mask + [T((2, 5), F, "opt")], extra=am, extra_required=True, nparam={4, 5, 6}, tag="[area]"))
    c.append(Case("md_pp_anchor_mask", mask, extra=am, extra_required=True, nparam={4, 5, 6}))
    return c


CASES = _cases()
