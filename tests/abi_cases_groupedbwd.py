"""One valid small call of md_conv2d_grouped_bwd_data and md_conv2d_grouped_bwd_weight (include/minddet_hip_groupedbwd.h) per
optional-operand form, in the form of tests/abi_cases.py (operand kinds and rank flags are explained there).  The feature's CPU test file
hands each row to the single-defect test of tests/abi_derive.py, and tests/test_abi_accept_gpu.py makes each row once on the GPU and
expects rc 0."""
import ctypes as C

from tests.abi_cases import B16, F, U8, Case, Grouped, T

G, COUT, Y_OFF, W_ROW, X_C_OFF = 2, (1, 3), (5, 1), (0, 2), 8        # dy of 8 channels, a pack of 6 rows (row 1 owned by no group)


def attrs(k=3):
    """two groups on channels 8 .. 135 of a 144-channel tensor: cout 1 at dy channel 5 / row 0, cout 3 at dy channels 1 .. 3 / rows 2 .. 4"""
    at = Grouped(k, 0, G, 64, X_C_OFF, 0)
    for g in range(G):
        at.cout[g], at.y_off[g], at.w_row[g] = COUT[g], Y_OFF[g], W_ROW[g]
    return at


def workspace_bytes(k):
    """per group one slab of 16 rows of k k 64 + 1 floats (P = 15)"""
    return G * 4 * 16 * (k * k * 64 + 1)


def _cases():
    c = []
    for k in (1, 3):
        for act in (True, False):
            ops = [T((1, 3, 5, 8), F), T((6, k * k * 64), B16), T((1, 3, 5, 144), B16, "opt", null=not act), T((1, 3, 5, 144), F)]
            c.append(Case("md_conv2d_grouped_bwd_data", ops, extra=attrs(k), extra_required=True, tag=f"[k{k}, {'act' if act else 'no act'}]"))
        for db in (True, False):
            ops = [T((1, 3, 5, 144), B16), T((1, 3, 5, 8), F), T((6, k * k * 64), F), T((6,), F, "opt", null=not db)]
            tag = f"k{k}" + ("" if db else ", no db")
            c.append(Case("md_conv2d_grouped_bwd_weight", ops, extra=attrs(k), extra_required=True, nparam={4, 5}, tag=f"[pool, {tag}]"))
            c.append(Case("md_conv2d_grouped_bwd_weight", ops + [T((workspace_bytes(k),), U8, "opt", "free")], extra=attrs(k), extra_required=True,
                          nparam={4, 5}, tag=f"[workspace, {tag}]"))
    return c


CASES = _cases()
assert C.sizeof(Grouped) == (6 + 3 * 64) * 4
