"""What tests/test_cp_augment_cpu.py, tests/test_cp_augment_gpu.py and tools share about the CenterPoint training input: the fixture
(tests/golden/cp_augment_vectors.npz) by case and the contract (tests/cpaug_contract.py) evaluated on it."""
import functools
import os

import numpy as np

from tests import cpaug_contract as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "cp_augment_vectors.npz")
NAMES = ("nusc", "flips0", "flips1", "flips2", "order", "plants")


@functools.lru_cache(maxsize=None)
def fixture_case(name):
    z = np.load(GOLD)
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}


def has_candidates(f):
    return "cand_boxes" in f


@functools.lru_cache(maxsize=None)
def contract_case(name):
    """the four contract stages on the fixture's inputs and draws (one sample) -> dict(count, accept, pts, boxes)"""
    f = fixture_case(name)
    G = len(f["gt_boxes"])
    cnt = cc.count_points(f["points"], f["gt_boxes"], G, int(f["min_points"]))
    if has_candidates(f):
        S = len(f["cand_boxes"])
        accept = cc.select(f["gt_boxes"], G, cnt["keep"], f["cand_boxes"], S, f["cand_group"])
        pts = cc.augment_points(f["points"], f["global"], f["cand_points"], f["cand_offsets"], f["cand_boxes"], accept)
        boxes = cc.augment_boxes(f["gt_boxes"], f["gt_classes"], G, cnt["keep"], f["global"], f["bv_range"], f["cand_boxes"], f["cand_classes"], accept)
    else:
        accept = None
        pts = cc.augment_points(f["points"], f["global"])
        boxes = cc.augment_boxes(f["gt_boxes"], f["gt_classes"], G, cnt["keep"], f["global"], f["bv_range"])
    return dict(count=cnt, accept=accept, pts=pts, boxes=boxes)
