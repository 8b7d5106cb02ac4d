"""Generate tests/golden/cn_target_vectors.npz FROM THE REFERENCE'S OWN COCOHP.preprocess_fn.

Run once in the build container (needs the reference checkout; never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/gen_cn_targets.py <path of the reference checkout>

Source of truth: minddet/models/centernet/src/dataset.py (COCOHP.preprocess_fn) with src/image.py, each loaded as a file under an
import-time shim: mindspore*, pycocotools* and src.model_utils.* are mocks and cv2 is a stub (the project does not depend on cv2) whose imdecode
returns a blank image of the wanted size, whose warpAffine returns zeros and whose getAffineTransform is this script's own float64
three-point solve, which records the matrix.  So the matrix itself and the image warp are NOT pinned by this fixture; everything behind
the matrix is: the flip, affine_transform, the clip, gaussian_radius, the Gaussian window and the five outputs.  preprocess_fn itself runs,
on an object.__new__(COCOHP), under seeded np.random; affine_transform is wrapped to record what it returned (the fp32 values the
reference then holds in `bbox`, before the clip).  Nothing of the reference is copied: the fixture holds seeded inputs and what the
reference's code returned for them.  The arithmetic recorded is the one of the NumPy that runs this script (>= 2: fp32 scalars stay
fp32); the version is stored in the file.

Cases
  small   B = 2, C = 5, 24 x 40 map (H x W), max_objs 32: sample 0 has 40 objects (truncated to 32) and is flipped, sample 1 has 14
          objects and is made with rand_crop
  tiles   B = 1, C = 3, 40 x 72 map, max_objs 32, scale / shift augmentation off: large boxes over the four corners (the clip cuts
          them; a Gaussian itself never reaches the map's edge: its radius is below the clipped box's half size) and across the
          64-column / 16-row borders of the heat-map kernel's tiles
  plants  B = 1, C = 3, 16 x 16 map, max_objs 32, identity matrix (the planted fp32 coordinates pass unchanged): edges clipped to
          exactly 0 and W - 1, a box wholly past an edge (w = 0: a zero slot between used ones), h in (0, 1], centres on an integer and
          on .5, radius 0, two objects of one class in one cell and two of different classes in one cell, overlapping Gaussians, a NaN
          coordinate, and rows of class 0, -1 and C + 1.  The reference has no padding rows (it would index hm[-1], hm[-2] or fail):
          for the run those three rows are given a degenerate box, which it skips leaving a zero slot -- the operator's documented
          rule for a padding row -- while the fixture's inputs carry a real box with the bad class.
"""
import importlib.util
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
f32 = np.float32
PKG = "minddet/models/centernet"
STATE = dict(image_hw=(0, 0), matrices=[], identity=False)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _three_point_solve(src, dst):
    """the 2 x 3 float64 matrix that maps the three src points onto the three dst points"""
    if STATE["identity"]:
        m = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    else:
        a = np.concatenate([np.asarray(src, np.float64), np.ones((3, 1))], 1)
        m = np.linalg.solve(a, np.asarray(dst, np.float64)).T.copy()
    STATE["matrices"].append(m)
    return m


def reference_dataset(ref_root):
    cv2 = types.ModuleType("cv2")
    cv2.IMREAD_COLOR, cv2.INTER_LINEAR, cv2.COLOR_BGR2GRAY = 1, 1, 6
    cv2.setNumThreads = lambda n: None
    cv2.imdecode = lambda buf, flag: np.zeros(STATE["image_hw"] + (3,), np.uint8)
    cv2.warpAffine = lambda img, m, size, flags=None: np.zeros((size[1], size[0], 3), np.uint8)
    cv2.getAffineTransform = _three_point_solve
    sys.modules["cv2"] = cv2
    for mock in ("mindspore", "mindspore.dataset", "mindspore.mindrecord", "pycocotools", "pycocotools.coco", "src.model_utils",
                 "src.model_utils.config", "src.model_utils.moxing_adapter"):
        sys.modules[mock] = MagicMock()
    pkg = types.ModuleType("src")
    pkg.__path__ = []
    sys.modules["src"] = pkg
    root = os.path.join(ref_root, PKG, "src")
    _load("src.image", os.path.join(root, "image.py"))
    return _load("src.dataset", os.path.join(root, "dataset.py"))


def run(ds, samples, num_classes, map_hw, max_objs, down_ratio=4):
    """preprocess_fn per sample -> the recorded inputs and returned arrays, stacked over the batch.  samples: dicts with image_hw,
    bboxes [n,4] f32, category_id [n], flip (bool), rand_crop (bool) and optionally run_bboxes (what the reference is given instead)"""
    record = []
    inner = sys.modules["src.image"].affine_transform

    def recording(pt, t):
        out = inner(pt, t)
        record.append(np.asarray(out, np.float64).astype(f32))      # what the assignment into the fp32 `bbox` keeps
        return out

    ds.affine_transform = recording
    G_in = max(len(s["bboxes"]) for s in samples)
    G_post = min(G_in, max_objs)
    B = len(samples)
    out = dict(bboxes=np.zeros((B, G_in, 4), f32), category_id=np.zeros((B, G_in), np.int32), num_objects=np.zeros(B, np.int32),
               trans_output=np.zeros((B, 2, 3)), flip_width=np.zeros(B, np.int32), post_boxes=np.zeros((B, G_post, 4), f32),
               post_classes=np.zeros((B, G_post), np.int32), hm=[], reg_mask=[], ind=[], wh=[], reg=[])
    for b, s in enumerate(samples):
        n = len(s["bboxes"])
        op = object.__new__(ds.COCOHP)
        op.run_mode = "train"
        op.data_opt = types.SimpleNamespace(max_objs=max_objs, input_res_train=(map_hw[0] * down_ratio, map_hw[1] * down_ratio),
                                            rand_crop=s["rand_crop"], scale=s.get("scale", 0.4), shift=s.get("shift", 0.1),
                                            flip_prop=1.0 if s["flip"] else 0.0,
                                            down_ratio=down_ratio, num_classes=num_classes, color_aug=False)
        op.net_opt = types.SimpleNamespace(mse_loss=False, dense_wh=False, cat_spec_wh=False, reg_offset=True)
        op.mean, op.std = np.zeros((1, 1, 3), f32), np.ones((1, 1, 3), f32)
        STATE["image_hw"], STATE["matrices"] = tuple(s["image_hw"]), []
        del record[:]
        given = np.array(s.get("run_bboxes", s["bboxes"]), f32)
        with np.errstate(invalid="ignore"):
            _, hm, reg_mask, ind, wh, reg = op.preprocess_fn(b"", n, given, np.array(s.get("run_category_id", s["category_id"]), np.int32))
        used = min(n, max_objs)
        assert len(record) == 2 * used and len(STATE["matrices"]) == 2
        out["bboxes"][b, :n], out["category_id"][b, :n], out["num_objects"][b] = s["bboxes"], s["category_id"], n
        out["trans_output"][b] = STATE["matrices"][1]
        out["flip_width"][b] = s["image_hw"][1] if s["flip"] else 0
        post = np.concatenate(record).reshape(used, 4)
        if "run_bboxes" in s:                                       # identity matrix: the planted boxes are their own post-affine values
            post = np.array(s["bboxes"], f32)[:used]
        out["post_boxes"][b, :used], out["post_classes"][b, :used] = post, s["category_id"][:used]
        for k, v in (("hm", hm), ("reg_mask", reg_mask), ("ind", ind.astype(np.int32)), ("wh", wh), ("reg", reg)):
            out[k].append(v)
    for k in ("hm", "reg_mask", "ind", "wh", "reg"):
        out[k] = np.stack(out[k])
    out["meta"] = np.array([num_classes, map_hw[0], map_hw[1], max_objs], np.int32)      # C, H, W, M
    return out


def seeded_boxes(rng, n, image_hw, size_lo, size_hi, classes):
    h, w = image_hw
    cx, cy = rng.uniform(-0.05 * w, 1.05 * w, n), rng.uniform(-0.05 * h, 1.05 * h, n)
    bw, bh = rng.uniform(size_lo, size_hi, n), rng.uniform(size_lo, size_hi, n)
    b = np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1).astype(f32)
    return b, rng.integers(1, classes + 1, n).astype(np.int32)


def case_small(ds, rng):
    b0, c0 = seeded_boxes(rng, 40, (120, 200), 2.0, 90.0, 5)
    b1, c1 = seeded_boxes(rng, 14, (480, 640), 8.0, 300.0, 5)
    return run(ds, [dict(image_hw=(120, 200), bboxes=b0, category_id=c0, flip=True, rand_crop=False),
                    dict(image_hw=(480, 640), bboxes=b1, category_id=c1, flip=False, rand_crop=True)], 5, (24, 40), 32)


def case_tiles(ds, rng):
    # a 160 x 288 image on a 40 x 72 map, scale and shift augmentation off: four image pixels per cell
    rows = [(-20, -20, 120, 90), (170, -30, 300, 70), (-10, 90, 110, 170), (180, 80, 300, 170),      # the four corners
            (200, 10, 310, 60), (230, 40, 280, 100), (100, 30, 270, 130), (240, 50, 262, 75),         # across column 64 (x = 256)
            (30, 40, 90, 90), (10, 50, 150, 80), (120, 100, 200, 150), (60, 110, 100, 145),            # across rows 16 and 32 (y = 64, 128)
            (0, 0, 288, 160), (140, 60, 148, 68), (250, 120, 259, 131), (254, 62, 258, 66)]
    b = np.array(rows, f32)
    c = (np.arange(len(rows)) % 3 + 1).astype(np.int32)
    return run(ds, [dict(image_hw=(160, 288), bboxes=b, category_id=c, flip=False, rand_crop=False, scale=0.0, shift=0.0)], 3, (40, 72), 32)


def case_plants(ds):
    nan = np.nan
    rows = [
        ((-3.0, 2.0, 4.0, 6.0), 1),          # 0  left edge clipped to exactly 0
        ((11.0, 3.0, 19.5, 9.0), 2),         # 1  right edge clipped to exactly W - 1 = 15
        ((16.5, 4.0, 22.0, 9.0), 1),         # 2  wholly past the right edge: both x clip to 15, w = 0 -> skipped, a zero slot
        ((5.0, 10.0, 9.0, 10.5), 3),         # 3  h = 0.5: ceil h = 1
        ((2.0, 12.0, 6.0, 13.0), 1),         # 4  h = 1 exactly; centre (4, 12.5): x on an integer, y on .5
        ((7.25, 7.25, 7.75, 7.75), 2),       # 5  radius 0 (a 1 x 1 box after the ceil)
        ((9.0, 1.0, 12.0, 4.0), 3),          # 6  two objects of class 3 in cell (10, 2) ...
        ((9.5, 1.5, 11.5, 3.5), 3),          # 7  ... with different sizes
        ((8.0, 0.0, 13.0, 5.0), 1),          # 8  and one of class 1 in the same cell
        ((1.0, 1.0, 8.0, 9.0), 2),           # 9  overlapping Gaussians of class 2 ...
        ((3.0, 2.0, 11.0, 8.0), 2),          # 10 ...
        ((nan, 3.0, 9.0, 8.0), 1),           # 11 a NaN coordinate: the size test fails
        ((4.0, 4.0, 9.0, 9.0), 0),           # 12 class 0
        ((5.0, 5.0, 10.0, 10.0), -1),        # 13 class -1
        ((6.0, 6.0, 12.0, 12.0), 4),         # 14 class C + 1
        ((0.0, 0.0, 15.0, 15.0), 1),         # 15 the whole map, behind the skipped rows
        ((-5.0, -5.0, 2.0, 0.75), 3),        # 16 top-left corner, h = 0.75 after the clip
    ]
    b = np.array([r[0] for r in rows], f32)
    c = np.array([r[1] for r in rows], np.int32)
    pad = (c < 1) | (c > 3)
    run_b, run_c = b.copy(), c.copy()
    run_b[pad], run_c[pad] = (2.0, 2.0, 2.0, 2.0), 1                # a degenerate box: the reference skips the row
    STATE["identity"] = True
    try:
        return run(ds, [dict(image_hw=(64, 64), bboxes=b, category_id=c, run_bboxes=run_b, run_category_id=run_c, flip=False,
                             rand_crop=False)], 3, (16, 16), 32)
    finally:
        STATE["identity"] = False


def main():
    ds = reference_dataset(sys.argv[1])
    np.random.seed(20260)
    rng = np.random.default_rng(20261)
    out = dict(numpy_version=np.array(np.__version__), min_overlap=np.float64(0.7))
    for name, case in (("small", case_small(ds, rng)), ("tiles", case_tiles(ds, rng)), ("plants", case_plants(ds))):
        for k, v in case.items():
            out[name + "_" + k] = v
        print(name, "objects", case["num_objects"].tolist(), "used slots", case["reg_mask"].sum(1).tolist(), "hm == 1 cells",
              int((case["hm"] == 1).sum()), "flip", case["flip_width"].tolist())
    path = os.path.join(HERE, "cn_target_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
