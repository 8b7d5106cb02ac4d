"""Generate tests/golden/cp_target_vectors.npz FROM THE REFERENCE'S OWN AssignLabel.

Run once in the build container (needs the reference checkout; never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/gen_cp_targets.py <path of the reference checkout>

Source of truth: minddet/models/centerpoint/det3d_ms/datasets/pipelines/preprocess.py (AssignLabel) with its numpy siblings
core/utils/center_utils.py, core/bbox/geometry.py and core/bbox/box_np_ops.py, each loaded as a file under an import-time shim:
numba.jit -> identity, det3d_ms.builder / the voxel generator / the sampler / circle_nms_jit -> mocks, and a PIPELINES registry whose
register_module is the identity.  Nothing of the reference is copied: the fixture holds seeded boxes and what AssignLabel.__call__
returned for them, per sample, stacked over the batch.  The arithmetic recorded is the one of the NumPy that runs this script
(>= 2: fp32 scalars stay fp32); the version is stored in the file.

Cases (0.2 m voxels, out_size_factor 4: 0.8 m cells; overlap 0.1, min_radius 2)
  small   B = 2, 24 x 20 map (W != H), tasks of 1, 2, 2 classes, max_objs 32, G = 24: 24 objects, and 9 objects + 15 padding rows
  tiles   B = 1, 72 x 40 map, tasks of 1, 2 classes, objects up to ~22 m (radius up to ~12) on the map's corners and edges and across
          the 64-column / 16-row borders of the heat-map kernel's tiles
  plants  B = 1, 16 x 16 map, tasks of 2, 1 classes: centres on a cell boundary and its fp32 neighbours, on the lower range edge
          (inside) and the upper one (outside), just below the lower edge (ct < 0 truncates to cell 0: the reference draws it); two
          objects of one class in one cell, overlapping Gaussians of one class and of two classes of one task; w = 0, l < 0, a class-0
          row in the middle, an id past the last class; headings +-pi (fp32), +-3 pi, +-7; an object whose radius falls below
          min_radius and one well above it
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
PKG = "minddet/models/centerpoint/det3d_ms"


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference_assign_label(ref_root):
    nb = types.ModuleType("numba")

    def _ident(*a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return a[0]
        return lambda f: f

    nb.jit = nb.njit = _ident
    sys.modules["numba"] = nb
    for pkg in ("det3d_ms", "det3d_ms.core", "det3d_ms.core.bbox", "det3d_ms.core.input", "det3d_ms.core.utils", "det3d_ms.datasets",
                "det3d_ms.datasets.pipelines"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    for mock in ("det3d_ms.builder", "det3d_ms.core.input.voxel_generator", "det3d_ms.core.sampler", "det3d_ms.core.sampler.preprocess",
                 "det3d_ms.core.utils.circle_nms_jit"):
        sys.modules[mock] = MagicMock()
    registry = types.ModuleType("det3d_ms.datasets.registry")
    registry.PIPELINES = types.SimpleNamespace(register_module=lambda cls: cls)
    sys.modules["det3d_ms.datasets.registry"] = registry
    root = os.path.join(ref_root, PKG)
    _load("det3d_ms.core.bbox.geometry", os.path.join(root, "core/bbox/geometry.py"))
    sys.modules["det3d_ms.core.bbox"].box_np_ops = _load("det3d_ms.core.bbox.box_np_ops", os.path.join(root, "core/bbox/box_np_ops.py"))
    _load("det3d_ms.core.utils.center_utils", os.path.join(root, "core/utils/center_utils.py"))
    return _load("det3d_ms.datasets.pipelines.preprocess", os.path.join(root, "datasets/pipelines/preprocess.py")).AssignLabel


CELL = dict(voxel_size=(0.2, 0.2), out_size_factor=4, gaussian_overlap=0.1, min_radius=2)


def run(AssignLabel, gt_boxes, gt_classes, num_classes, pc_range, wh, max_objs):
    """AssignLabel.__call__ per sample -> the returned arrays stacked over the batch"""
    tasks = [types.SimpleNamespace(num_class=n, class_names=["c%d_%d" % (t, i) for i in range(n)]) for t, n in enumerate(num_classes)]
    cfg = types.SimpleNamespace(out_size_factor=CELL["out_size_factor"], target_assigner=types.SimpleNamespace(tasks=tasks),
                                gaussian_overlap=CELL["gaussian_overlap"], max_objs=max_objs, min_radius=CELL["min_radius"])
    op = AssignLabel(cfg=cfg)
    out = {k: [] for k in ("hm", "anno_box", "ind", "mask", "cat", "gt_boxes_and_cls")}
    for boxes, classes in zip(gt_boxes, gt_classes):
        voxels = dict(shape=np.array([wh[0] * CELL["out_size_factor"], wh[1] * CELL["out_size_factor"], 1], np.int64),
                      range=np.array([pc_range[0], pc_range[1], -5.0, 0, 0, 3.0], f32), size=np.array(CELL["voxel_size"] + (8.0,), f32))
        ann = dict(gt_boxes=boxes.copy(), gt_classes=classes.astype(np.int64), gt_names=np.array(["n"] * len(classes)))
        res = dict(mode="train", type="NuScenesDataset", lidar=dict(voxels=voxels, annotations=ann))
        res, _ = op(res, None)
        ex = res["lidar"]["targets"]
        for k in out:
            out[k].append(np.stack(ex[k]) if isinstance(ex[k], list) else ex[k])
    return {k: np.stack(v) for k, v in out.items()}


def seeded(rng, n, lo, hi, size_lo, size_hi, classes):
    b = np.zeros((n, 9), f32)
    b[:, 0] = rng.uniform(lo[0] - 0.4, hi[0] + 0.4, n)
    b[:, 1] = rng.uniform(lo[1] - 0.4, hi[1] + 0.4, n)
    b[:, 2] = rng.uniform(-3, 1, n)
    b[:, 3:5] = rng.uniform(size_lo, size_hi, (n, 2))
    b[:, 5] = rng.uniform(0.5, 3.5, n)
    b[:, 6:8] = rng.normal(0, 3, (n, 2))
    b[:, 8] = rng.uniform(-4.0, 4.0, n)
    return b, rng.integers(1, classes + 1, n).astype(np.int32)


def case_small(rng):
    lo, hi = (-9.6, -8.0), (9.6, 8.0)
    b0, c0 = seeded(rng, 24, lo, hi, 0.4, 5.0, 5)
    b1, c1 = seeded(rng, 9, lo, hi, 0.4, 5.0, 5)
    b1 = np.concatenate([b1, np.zeros((15, 9), f32)])
    c1 = np.concatenate([c1, np.zeros(15, np.int32)])
    p = rng.permutation(24)                       # padding rows anywhere, not only at the end
    return np.stack([b0, b1[p]]), np.stack([c0, c1[p]]), [1, 2, 2], lo, (24, 20), 32


def case_tiles(rng):
    lo = (-28.8, -16.0)                            # 72 x 40 cells of 0.8 m
    rows = []

    def at(cx, cy, size, cls):                    # centre in cells
        rows.append(([lo[0] + 0.8 * cx, lo[1] + 0.8 * cy, rng.uniform(-2, 1), size * rng.uniform(0.9, 1.0), size, rng.uniform(1, 3),
                      rng.normal(), rng.normal(), rng.uniform(-3.1, 3.1)], cls))

    for cx, cy in ((0.5, 0.5), (71.5, 0.5), (0.5, 39.5), (71.5, 39.5)):          # corners
        at(cx, cy, 22.0, 1)
    for cx, cy in ((36.2, 0.3), (36.7, 39.9), (0.1, 20.5), (71.9, 19.5)):        # edges
        at(cx, cy, 14.0, 2)
    for cx, cy in ((63.9, 15.9), (64.1, 16.1), (63.5, 31.5), (64.5, 32.5), (60.5, 8.5), (67.5, 24.5)):   # tile borders
        at(cx, cy, 18.0, 3)
    for cx, cy in ((20.5, 15.5), (40.5, 16.5), (63.2, 20.2), (64.8, 12.7)):
        at(cx, cy, 6.0, int(rng.integers(1, 4)))
    for _ in range(6):
        at(rng.uniform(0, 72), rng.uniform(0, 40), rng.uniform(1.0, 22.0), int(rng.integers(1, 4)))
    p = rng.permutation(len(rows))
    b = np.asarray([rows[i][0] for i in p], f32)
    c = np.asarray([rows[i][1] for i in p], np.int32)
    return b[None], c[None], [1, 2], lo, (72, 40), 40


def case_plants():
    lo, up = f32(-6.4), f32(6.4)
    rows = []

    def add(x, y, w=1.6, l=2.4, cls=1, rot=0.3, z=-1.0, h=1.5):
        rows.append(([x, y, z, w, l, h, 0.5, -0.25, rot], cls))

    e = f32((f32(5) * f32(0.8)) + lo)              # a cell boundary as fp32 arithmetic gives it
    for v in (e, np.nextafter(e, f32(-100)), np.nextafter(e, f32(100)), f32(-6.4 + 5 * 0.8)):
        add(v, 2.0)
        add(-3.0, v, cls=2)
    add(lo, 0.1)                                   # lower range edge: inside
    add(0.1, lo, cls=3)
    add(up, 0.1)                                   # upper range edge: outside
    add(0.1, up, cls=3)
    add(np.nextafter(lo, f32(-100)), 3.3)          # just below the lower edge: ct < 0, ct_int = 0
    add(3.3, np.nextafter(lo, f32(-100)), cls=2)
    add(f32(-7.0), 1.0)                            # a cell below the range: ct_int = 0 as well
    add(f32(-7.3), 1.0)                            # ct = -1.125: ct_int = -1, out
    add(2.1, -4.1, cls=3)                          # two objects of one class in one cell
    add(2.3, -4.3, cls=3, w=2.0)
    add(4.0, 4.0, w=8.0, l=8.0)                    # overlapping Gaussians, one class
    add(5.7, 4.9, w=6.0, l=9.0)
    add(-4.0, 4.0, w=8.0, l=6.0, cls=1)            # overlapping Gaussians, two classes of one task
    add(-3.1, 3.2, w=7.0, l=7.0, cls=2)
    add(1.0, 1.0, w=0.0)                           # degenerate rows
    add(1.0, 1.0, l=-1.0, cls=2)
    add(0.0, 0.0, cls=0)
    add(0.0, 0.0, cls=4)
    add(0.0, 0.0, cls=-1)
    for i, r in enumerate((f32(np.pi), -f32(np.pi), f32(3 * np.pi), f32(-3 * np.pi), f32(7.0), f32(-7.0), f32(0.0), f32(100.0))):
        add(-5.0 + 1.2 * i, -1.5, rot=r, cls=1 + i % 3)
    add(-1.0, 5.0, w=0.5, l=0.5, cls=3)            # radius below min_radius
    add(0.5, -5.5, w=12.0, l=10.0, cls=2)          # radius well above it
    b = np.asarray([r[0] for r in rows], f32)
    c = np.asarray([r[1] for r in rows], np.int32)
    return b[None], c[None], [2, 1], (-6.4, -6.4), (16, 16), 48


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    AssignLabel = reference_assign_label(sys.argv[1])
    rng = np.random.default_rng(20241018)
    cases = dict(small=case_small(rng), tiles=case_tiles(rng), plants=case_plants())
    out = dict(cases=np.asarray(sorted(cases)), numpy_version=np.asarray(np.__version__))
    for k, v in CELL.items():
        out[k] = np.asarray(v, np.int32 if isinstance(v, int) else np.float64)
    for name, (boxes, classes, num_classes, lo, wh, max_objs) in cases.items():
        got = run(AssignLabel, boxes, classes, num_classes, lo, wh, max_objs)
        out[name + "_gt_boxes"], out[name + "_gt_classes"] = boxes, classes
        out[name + "_num_classes"], out[name + "_pc_range"] = np.asarray(num_classes, np.int32), np.asarray(lo, np.float64)
        out[name + "_feature_map_size"], out[name + "_max_objs"] = np.asarray(wh, np.int32), np.int32(max_objs)
        for k, v in got.items():
            assert v.dtype in (np.float32, np.uint8, np.int64), (k, v.dtype)
            out[name + "_" + k] = v.astype(np.int32) if v.dtype == np.int64 else v
        drawn = int(got["mask"].sum())
        dup = sum(int(m.sum()) - len(np.unique(i[m > 0])) for i, m in zip(got["ind"].reshape(-1, max_objs), got["mask"].reshape(-1, max_objs)))
        members = int((got["gt_boxes_and_cls"][..., 9] > 0).sum())
        print(name, "members", members, "drawn", drawn, "sharing a cell", dup, "hm non-zero", int((got["hm"] > 0).sum()))
        if name == "small":                          # the round-trip test leaves objects that share a cell out: at most a quarter
            shared = 0
            for i, m in zip(got["ind"].reshape(-1, max_objs), got["mask"].reshape(-1, max_objs)):
                u, n = np.unique(i[m > 0], return_counts=True)
                shared += int(n[n > 1].sum())
            assert 4 * shared <= drawn, (shared, drawn)
    dst = os.path.join(HERE, "cp_target_vectors.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes; numpy", np.__version__)


if __name__ == "__main__":
    main()
