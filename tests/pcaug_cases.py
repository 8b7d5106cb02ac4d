"""What tests/test_pc_augment_cpu.py, tests/test_pc_augment_gpu.py and tools share about the KITTI training augmentation: the fixture
(tests/golden/pc_augment_vectors.npz) by case, the contract (tests/pcaug_contract.py) evaluated on it, and the single-defect calls of
tests/test_abi_checks_cpu.py for rows with float64 operands (that module's table of item sizes has no float64 and its "wrong dtype"
is float64; nothing of it is changed here: the calls are copied into a Call that knows the size, and the wrong dtype of a float64
operand is float32)."""
import copy
import ctypes as C
import functools
import os

import numpy as np

from tests import pcaug_contract as pc
from tests import test_abi_checks_cpu as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "pc_augment_vectors.npz")
NAMES = ("car", "nogrot", "pedcyc")
F64 = "float64"
ITEM = dict(abi.ITEM, float64=8)


@functools.lru_cache(maxsize=None)
def fixture_case(name):
    z = np.load(GOLD)
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}


@functools.lru_cache(maxsize=None)
def contract_case(name):
    """the three contract stages on the fixture's inputs and draws (one sample) -> dict"""
    f = fixture_case(name)
    G = len(f["gt_boxes"])
    grot = f["grot"] if "grot" in f else None
    sel, tf, moved = pc.noise_per_object(f["gt_boxes"], G, f["valid"], f["loc"], f["rot"], grot)
    terr = pc.transform_bound(f["gt_boxes"], G, sel, grot is not None)
    R = len(f["remove_boxes"])
    pts = pc.augment_points(f["points"], f["gt_boxes"], G, f["valid"], tf, f["global"], f["remove_boxes"] if R else None, R,
                            int(f["remove_from"]), box_err=terr)
    in_err = np.zeros((G, 7))
    in_err[:, 0] = in_err[:, 1] = terr + pc.U * np.abs(moved[:, :2]).max(1)
    in_err[:, 2] = pc.U * np.abs(moved[:, 2])
    in_err[:, 6] = pc.U * np.abs(moved[:, 6])
    boxes = pc.augment_boxes(moved, G, f["valid"], f["classes"], f["global"], f["bv_range"], in_err=in_err)
    return dict(selected=sel, tf=tf, moved=moved, terr=terr, pts=pts, boxes=boxes)


def reference_owner(f):
    """[N] the reference's decision per input point: -2 dropped by remove_points_in_boxes, else the first valid box whose mask holds, -1"""
    nf, n = int(f["remove_from"]), len(f["points"])
    drop = np.concatenate([np.zeros(nf, bool), f["removed"]]) if len(f["remove_boxes"]) else np.zeros(n, bool)
    masks = f["point_masks"] & (f["valid"] != 0)[None]
    own = np.full(n, -2, np.int32)
    own[~drop] = np.where(masks.any(1), masks.argmax(1), -1)
    return own


class Call64(abi.Call):
    """abi.Call with an item size for float64 (run() is that class's, with this module's table)"""

    def run(self, lib):
        n = self.n
        ops = self.case.operands
        sizes = [max(64, ITEM[t.dtype] * max(1, abi._numel(t.shape)) + 64) for t in ops] + [64] * (n - len(ops))
        arena = (C.c_char * sum(sizes))()
        base, off = C.addressof(arena), 0
        params, ndims = (C.c_void_p * n)(), (C.c_int * n)()
        shapes, dtypes = (C.POINTER(C.c_int64) * n)(), (C.c_char_p * n)()
        keep = []
        for i in range(n):
            described = i < len(self.shapes)
            params[i] = None if (described and self.null_ptr[i]) else base + off
            off += sizes[i]
            shp = ([] if ops[i].null else self.shapes[i]) if described else [64]
            ndims[i] = len(shp)
            buf = (C.c_int64 * max(len(shp), 1))(*shp)
            keep.append(buf)
            shapes[i] = None if (described and self.null_shape[i]) else C.cast(buf, C.POINTER(C.c_int64))
            dtypes[i] = self.dtypes[i] if described else b"uint8"
        extra = None if (self.case.extra is None or self.extra_null) else C.byref(self.case.extra)
        return getattr(lib, self.case.sym)(n, None if self.params_null else params, None if self.ndims_null else ndims,
                                           None if self.shapes_null else shapes, None if self.dtypes_null else dtypes, None, extra)


def mutations64(case):
    """abi.mutations(case) as Call64 objects; the wrong dtype of a float64 operand is float32"""
    out = []
    for kind, i, call, want in abi.mutations(case):
        c = Call64.__new__(Call64)
        c.__dict__.update(call.__dict__)
        if kind == "dtype" and case.operands[i].dtype == F64:
            c.dtypes[i] = b"float32"
        out.append((kind, i, c, want))
    return out


def edited(case, edit):
    """a Call64 of `case` after edit(copy of the case)"""
    c = copy.copy(case)
    if case.extra is not None:
        c.extra = type(case.extra).from_buffer_copy(case.extra)
    c.operands = list(case.operands)
    edit(c)
    return Call64(c)
