"""One valid small call per MD_AOT_ARGS entry point of include/minddet_hip_points.h, in the form of tests/abi_cases.py (operand kinds and
rank flags are explained there).  The feature's CPU test file hands each row to the single-defect test of tests/abi_derive.py, and
tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0."""
from tests.abi_cases import B16, F, I, U8, Case, S, T, f32, i32   # noqa: F401

Voxelize = S(("voxel_size", f32 * 3), ("range", f32 * 6), ("max_points", i32), ("max_voxels", i32))
PillarEncode = S(("vx", f32), ("vy", f32), ("x_offset", f32), ("y_offset", f32), ("with_distance", i32), ("virtual_points", i32))


def _cases():
    c = []
    vox = Voxelize((f32 * 3)(0.2, 0.2, 8.0), (f32 * 6)(-1.6, -1.6, -5.0, 1.6, 1.6, 3.0), 4, 8)
    c.append(Case("md_voxelize", [T((16, 5), F), T((3,), I), T((2, 8, 4, 5), F), T((2, 8, 4), I), T((2, 8), I), T((2,), I)], extra=vox,
                  extra_required=True, nparam={6, 7}))
    enc = PillarEncode(0.2, 0.2, -1.5, -1.5, 0, 0)
    ops = [T((2, 8, 4, 5), F), T((2, 8), I), T((2, 8, 4), I), T((2,), I)]
    c.append(Case("md_pillar_encode", ops + [T((32, 10), F), T((32,), F), T((64, 64), F, "opt"), T((64,), F, "opt"), T((2, 16, 16, 64), B16)],
                  extra=enc, extra_required=True, tag="[two]"))
    c.append(Case("md_pillar_encode", ops + [T((64, 10), F), T((64,), F), T((64, 64), F, "opt", null=True), T((64,), F, "opt", null=True),
                                             T((2, 16, 16, 64), B16)], extra=enc, extra_required=True, tag="[one]"))
    return c


CASES = _cases()
