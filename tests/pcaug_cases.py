"""What tests/test_pc_augment_cpu.py, tests/test_pc_augment_gpu.py and tools share about the KITTI training augmentation: the fixture
(tests/golden/pc_augment_vectors.npz) by case, the contract (tests/pcaug_contract.py) evaluated on it, and the reference's decision
per point."""
import functools
import os

import numpy as np

from tests import pcaug_contract as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "pc_augment_vectors.npz")
NAMES = ("car", "nogrot", "pedcyc")


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
