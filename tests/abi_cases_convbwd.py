"""One valid small call of md_conv_bwd_weight and md_conv1x1_bwd_data (include/minddet_hip_convbwd.h) per optional-operand form, in the
form of tests/abi_cases.py (operand kinds and rank flags are explained there).  The feature's CPU test file hands each row to the
single-defect test of tests/abi_derive.py, and tests/test_abi_accept_gpu.py makes each row once on the GPU and expects rc 0."""
import ctypes as C

from tests.abi_cases import B16, F, U8, Case, S, T, i32

Block = S(*[(n, i32) for n in ("row0", "rows", "col0", "cols")])
ConvBwd = S(*[(n, i32) for n in ("cin", "cout", "x_c_off", "dy_c_off", "kernel", "korder", "n_blocks")], ("blocks", Block * 4), ("reserved0", i32))
Conv1x1BwdData = S(*[(n, i32) for n in ("cin", "cout", "dy_c_off", "dx_c_off", "act_c_off", "reserved0")])


def wgrad_attrs(kernel=3, n_blocks=0):
    """cin 8 of the 16 channels of x from channel 8 on, cout 3 of the 8 channels of dy from channel 2 on; one block: rows 1 .. 2, all
    input channels"""
    at = ConvBwd(8, 3, 8, 2, kernel, 0, n_blocks)
    at.blocks[0] = Block(1, 2, 0, 8)
    return at


def dgrad_attrs(act):
    """cin 8 at channels 4 .. 11 of dx (and of act), cout 3 of the 8 channels of dy from channel 2 on"""
    return Conv1x1BwdData(8, 3, 2, 4, 4 if act else 0, 0)


def _wgrad_operands(db, kernel):
    # N = 1, a 3 x 5 map: P = 15 pixels; dw [32, 128] holds the pack of an 8 -> 3 layer of either kernel, db its bias
    return [T((1, 3, 5, 16), B16), T((1, 3, 5, 8), F), T((32, 128), F), T((32,), F, "opt", null=not db)]


def workspace_bytes(kernel):
    """one slab of R = 16 rows of kernel^2 cin + 1 floats"""
    return 4 * 16 * (kernel * kernel * 8 + 1)


def _cases():
    c = []
    for kernel in (1, 3):
        for db in (True, False):
            tag = f"k{kernel}" + ("" if db else ", no db")
            c.append(Case("md_conv_bwd_weight", _wgrad_operands(db, kernel), extra=wgrad_attrs(kernel), extra_required=True, nparam={4, 5},
                          tag=f"[pool, {tag}]"))
            c.append(Case("md_conv_bwd_weight", _wgrad_operands(db, kernel) + [T((workspace_bytes(kernel),), U8, "opt", "free")],
                          extra=wgrad_attrs(kernel), extra_required=True, nparam={4, 5}, tag=f"[workspace, {tag}]"))
    c.append(Case("md_conv_bwd_weight", _wgrad_operands(True, 3), extra=wgrad_attrs(3, n_blocks=1), extra_required=True, nparam={4, 5},
                  tag="[pool, k3, one block]"))
    for act in (True, False):
        ops = [T((1, 3, 5, 8), F), T((32, 64), B16), T((1, 3, 5, 12), B16, "opt", null=not act), T((1, 3, 5, 12), F)]
        c.append(Case("md_conv1x1_bwd_data", ops, extra=dgrad_attrs(act), extra_required=True, tag="[act]" if act else "[no act]"))
    return c


CASES = _cases()
assert C.sizeof(ConvBwd) == 24 * 4
