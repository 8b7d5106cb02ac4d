"""Golden vectors for the CenterPoint training input, produced BY THE REFERENCE: the training branch of Preprocess.__call__ and the
ground-truth filter of Voxelization.__call__ (minddet/models/centerpoint/det3d_ms/datasets/pipelines/preprocess.py:46-157, 187-193)
driven step by step, in that order, with the reference's own routines: box_np_ops.points_count_rbbox, DataBaseSamplerV2.sample_all
(an in-memory db_infos, the objects' points as .bin files in a temporary directory), random_flip_both, global_rotation,
global_scaling_v2, global_translate_, filter_gt_box_outside_range.  core/bbox/geometry.py, core/bbox/box_np_ops.py,
core/sampler/preprocess.py and core/sampler/sample_ops.py are loaded as files under the numba-identity shim of gen_cp_targets.py.
numpy's generator is seeded and np.random.normal / uniform / choice are wrapped during the calls (Capture of gen_pc_augment.py), so
the float64 draws the reference used are recorded and become the operators' inputs.  Run here only:

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/gen_cp_augment.py <path of the reference checkout>

Nothing of the reference is copied: the file holds seeded inputs, the draws and what the routines returned.

Asserted while generating: (i) outside `plants` every point-in-box and corner-in-range decision's margin is above the contract's
MARGIN and the contract decides as the reference did; in `plants` the undecided decisions are exactly the planted ones; (ii) on every
pair that box_collision_test is called on, its result on the fp32 corners equals the contract's predicate on float64 corners -- under
the shim the reference's identity comparison skips the containment tests (quirk (a)), so this also says that in no pair of the fixture
the two readings differ; a containment-only pair is tested against the contract alone (tests/test_cp_augment_gpu.py); (iii) the
contract's select equals the candidates sample_all returned.
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True
from gen_cp_targets import PKG, _load  # noqa: E402
from gen_pc_augment import Capture  # noqa: E402

BV_RANGE = np.array([-51.2, -51.2, 51.2, 51.2], np.float32)
CLASS_NAMES = ["car", "truck", "pedestrian"]          # the global class of a name is its index + 1
SIZES = dict(car=(1.9, 4.6, 1.7), truck=(2.5, 7.0, 2.8), pedestrian=(0.7, 0.7, 1.8), animal=(0.5, 1.0, 0.6))


def reference_modules(ref_root):
    nb = types.ModuleType("numba")

    def _ident(*a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return a[0]
        return lambda f: f

    nb.jit = nb.njit = _ident
    sys.modules["numba"] = nb
    for pkg in ("det3d_ms", "det3d_ms.core", "det3d_ms.core.bbox", "det3d_ms.core.sampler"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    root = os.path.join(ref_root, PKG)
    _load("det3d_ms.core.bbox.geometry", os.path.join(root, "core/bbox/geometry.py"))
    ops = _load("det3d_ms.core.bbox.box_np_ops", os.path.join(root, "core/bbox/box_np_ops.py"))
    sys.modules["det3d_ms.core.bbox"].box_np_ops = ops
    prep = _load("det3d_ms.core.sampler.preprocess", os.path.join(root, "core/sampler/preprocess.py"))
    sys.modules["det3d_ms.core.sampler"].preprocess = prep
    sops = _load("det3d_ms.core.sampler.sample_ops", os.path.join(root, "core/sampler/sample_ops.py"))
    return ops, prep, sops


def to_lidar(local, box):
    """points in a box's frame (x along w, y along l, z from the centre) -> lidar, float64"""
    c, s = np.cos(np.float64(box[8])), np.sin(np.float64(box[8]))
    x = local[:, 0] * c + local[:, 1] * s + np.float64(box[0])
    y = -local[:, 0] * s + local[:, 1] * c + np.float64(box[1])
    return np.stack([x, y, local[:, 2] + np.float64(box[2])], 1)


def make_box(rng, name, x, y, r=None):
    w, l, h = SIZES[name]
    return np.array([x, y, rng.uniform(-1.2, -0.8), w * rng.uniform(0.9, 1.1), l * rng.uniform(0.9, 1.1), h, rng.uniform(-3, 3), rng.uniform(-3, 3),
                     rng.uniform(-np.pi, np.pi) if r is None else r], np.float32)


def inner_points(rng, box, n, F=5):
    loc = np.stack([rng.uniform(-0.45, 0.45, n) * box[3], rng.uniform(-0.45, 0.45, n) * box[4], rng.uniform(-0.45, 0.45, n) * box[5]], 1)
    return np.concatenate([to_lidar(loc, box), rng.uniform(0, 1, (n, F - 3))], 1).astype(np.float32)


def drive(mods, tmp, name, seed, points, gt_boxes, gt_names, db, groups, min_points, rot, scale, std, keep_order=False, plants=None):
    """the steps of Preprocess.__call__ (train) and Voxelization.__call__ (train) on one sample -> the case's arrays"""
    ops, prep, sops = mods
    from tests import cpaug_contract as cc

    np.random.seed(seed)
    G = len(gt_boxes)
    out = dict(points=points.copy(), gt_boxes=gt_boxes.copy(), bv_range=BV_RANGE, min_points=np.int32(min_points),
               gt_classes=np.array([CLASS_NAMES.index(n) + 1 if n in CLASS_NAMES else 0 for n in gt_names], np.int32))
    gt_dict = dict(gt_boxes=gt_boxes.copy(), gt_names=np.array(gt_names))
    pts = points.copy()
    counts = ops.points_count_rbbox(pts, gt_dict["gt_boxes"])
    keep = counts >= min_points if min_points > 0 else np.ones(G, bool)
    out.update(counts=np.asarray(counts, np.int32), keep=keep.astype(np.uint8))
    c = cc.count_points(points, gt_boxes, G, min_points)
    undecided = {(int(i), int(g)) for i, g in zip(*np.nonzero(c["margin"] <= cc.MARGIN))}
    assert undecided == set(plants["pairs"] if plants else ()), f"{name}: undecided point / box pairs {sorted(undecided)}"      # (i)
    assert ((counts >= c["lo"]) & (counts <= c["hi"])).all() and np.array_equal(c["keep"][c["keep_decided"]], out["keep"][c["keep_decided"]])
    gt_dict = {k: v[keep] for k, v in gt_dict.items()}
    gt_boxes_mask = np.array([n in CLASS_NAMES for n in gt_dict["gt_names"]], dtype=np.bool_)

    S = 0
    if db is not None:
        files = {}
        for cls, infos in db.items():
            for k, info in enumerate(infos):
                info["path"] = f"{name}_{cls}_{k}.bin"
                info["uid"] = f"{cls}_{k}"
                files[info["uid"]] = info.pop("points")
                files[info["uid"]].tofile(os.path.join(tmp, info["path"]))
        logger = types.SimpleNamespace(info=lambda *a, **k: None)
        sampler = sops.DataBaseSamplerV2(db, groups, db_prepor=None, rate=1.0, global_rot_range=[0, 0], logger=logger)
        assert not sampler.use_group_sampling and not sampler._enable_global_rot
        drawn = []
        for cls, bs in sampler._sampler_dict.items():
            if keep_order:
                bs._indices = np.arange(len(bs._indices))
            real_sample = bs.sample

            def recording(num, real_sample=real_sample):
                got = real_sample(num)
                drawn.append(got)
                return got
            bs.sample = recording
        real_coll = prep.box_collision_test

        def colliding(boxes, qboxes, clockwise=True):
            ret = real_coll(boxes, qboxes, clockwise)
            b64 = boxes.astype(np.float64)
            hit = cc.collide(b64[:, None, :, 0], b64[:, None, :, 1], b64[None, :, :, 0], b64[None, :, :, 1])[3]
            assert np.array_equal(ret, hit), f"{name}: box_collision_test and the contract's predicate differ"          # (ii), first half
            return ret
        prep.box_collision_test = colliding
        try:
            sampled = sampler.sample_all(tmp, gt_dict["gt_boxes"], gt_dict["gt_names"], 5, False, gt_group_ids=None, calib=None, road_planes=None)
        finally:
            prep.box_collision_test = real_coll
        cand = [info for call in drawn for info in call]
        S = len(cand)
        cand_boxes = np.stack([i["box3d_lidar"] for i in cand]).astype(np.float32)
        cand_group = np.concatenate([np.full(len(call), k, np.int32) for k, call in enumerate(drawn)])
        cand_classes = np.array([CLASS_NAMES.index(i["name"]) + 1 if i["name"] in CLASS_NAMES else 0 for i in cand], np.int32)
        cand_points = np.concatenate([files[i["uid"]] for i in cand], 0)
        cand_offsets = np.concatenate([[0], np.cumsum([len(files[i["uid"]]) for i in cand])]).astype(np.int32)
        accept = np.zeros(S, np.uint8)
        # which candidates came back: sample_all keeps their order, and a returned box is its candidate's box bit for bit
        ret_boxes = np.zeros((0, 9), np.float32) if sampled is None else sampled["gt_boxes"]
        k = 0
        for s in range(S):
            if k < len(ret_boxes) and np.array_equal(ret_boxes[k], cand_boxes[s]):
                accept[s] = 1
                k += 1
        assert k == len(ret_boxes)
        # (ii), second half: the float64 corners from the fp32 boxes give the same matrix as the reference's fp32 corners did, and (iii)
        assert np.array_equal(cc.select(gt_boxes, G, out["keep"], cand_boxes, S, cand_group), accept), f"{name}: select differs"
        out.update(cand_boxes=cand_boxes, cand_group=cand_group, cand_classes=cand_classes, cand_points=cand_points, cand_offsets=cand_offsets,
                   accept=accept)
        if sampled is not None:
            gt_dict["gt_names"] = np.concatenate([gt_dict["gt_names"], sampled["gt_names"]], axis=0)
            gt_dict["gt_boxes"] = np.concatenate([gt_dict["gt_boxes"], sampled["gt_boxes"]])
            gt_boxes_mask = np.concatenate([gt_boxes_mask, sampled["gt_masks"]], axis=0)
            pts = np.concatenate([sampled["points"], pts], axis=0)
    gt_dict = {k: v[gt_boxes_mask] for k, v in gt_dict.items()}
    classes = np.array([CLASS_NAMES.index(n) + 1 for n in gt_dict["gt_names"]], dtype=np.int32)
    boxes = gt_dict["gt_boxes"].astype(np.float32)
    out.update(points_merged=pts.copy(), boxes_merged=boxes.copy(), classes_merged=classes)
    with Capture() as cap:
        boxes, pts = prep.random_flip_both(boxes, pts)
        out.update(boxes_flip=boxes.copy(), points_flip=pts.copy())
        boxes, pts = prep.global_rotation(boxes, pts, rotation=list(rot))
        out.update(boxes_rot=boxes.copy(), points_rot=pts.copy())
        boxes, pts = prep.global_scaling_v2(boxes, pts, *scale)
        out.update(boxes_scale=boxes.copy(), points_scale=pts.copy())
        boxes, pts = prep.global_translate_(boxes, pts, noise_translate_std=std)
        out.update(boxes_translate=boxes.copy(), points_translate=pts.copy())
    kinds = [k for k, _, _ in cap.draws]
    assert kinds == ["choice", "choice", "uniform", "uniform"] + (["normal"] * 3 if std else []), kinds
    vals = [float(np.asarray(c).reshape(-1)[0]) for _, _, c in cap.draws] + ([] if std else [0.0, 0.0, 0.0])
    out["global"] = np.array(vals, np.float64)
    mask = prep.filter_gt_box_outside_range(boxes, BV_RANGE)
    out.update(range_mask=mask, final_boxes=boxes[mask], final_classes=classes[mask])
    assert boxes.dtype == pts.dtype == np.float32 and pts.shape[1] == 5
    b = cc.augment_boxes(gt_boxes, out["gt_classes"], G, out["keep"], out["global"], BV_RANGE, *([out["cand_boxes"], out["cand_classes"], out["accept"]]
                                                                                                 if S else []))
    und = set(np.flatnonzero(b["margin"] <= cc.MARGIN).tolist())
    assert und == set(plants["range_rows"] if plants else ()), f"{name}: undecided range rows {sorted(und)}"                   # (i)
    dec = b["margin"] > cc.MARGIN
    assert len(b["mask"]) == len(mask) and np.array_equal(b["mask"][dec], mask[dec])
    return {f"{name}_{k}": v for k, v in out.items()}, out


def scene(rng, names, n_inside, n_bg, extent=46.0, far=()):
    """ground truth on a jittered grid (no two overlap), n_inside[g] points inside row g, background points above every box"""
    G = len(names)
    cells = [(x, y) for x in np.arange(-extent + 6, extent, 12.0) for y in np.arange(-extent + 6, extent, 12.0)]
    pick = rng.permutation(len(cells))[:G]
    boxes = np.stack([make_box(rng, names[g], cells[k][0] + rng.uniform(-1, 1), cells[k][1] + rng.uniform(-1, 1)) for g, k in enumerate(pick)])
    for g, xy in far:
        boxes[g, :2] = xy
    pts = [inner_points(rng, boxes[g], n_inside[g]) for g in range(G)]
    bg = np.stack([rng.uniform(-51, 51, n_bg), rng.uniform(-51, 51, n_bg), rng.uniform(1.5, 3.0, n_bg), rng.uniform(0, 1, n_bg), rng.uniform(0, 0.5, n_bg)], 1)
    points = np.concatenate(pts + [bg.astype(np.float32)], 0)
    return boxes, points[rng.permutation(len(points))], cells, set(pick.tolist())


def database(rng, per_class, where):
    """db_infos: per class a list of dict(name, box3d_lidar [9] f32, points [n, 5] f32 in the object's frame, difficulty)"""
    db = {}
    for cls, n in per_class.items():
        infos = []
        for k in range(n):
            x, y = where(cls, k)
            box = make_box(rng, cls, x, y)
            m = int(rng.integers(3, 40))
            loc = inner_points(rng, np.array([0, 0, 0, box[3], box[4], box[5], 0, 0, 0], np.float32), m)
            infos.append(dict(name=cls, box3d_lidar=box, points=loc, difficulty=0, num_points_in_gt=m))
        db[cls] = infos
    return db


def case_scene(mods, tmp, name, seed, G, n_draw, n_points, want_flips, min_points, std):
    """a scene with a database; the seed is walked until the two flips come out as wanted and every assertion holds"""
    for sd in range(seed, seed + 400):
        rng = np.random.default_rng(sd)
        names = (["car", "truck", "pedestrian", "animal"] * G)[:G]
        if name == "nusc":
            names = ["car"] * 5 + ["truck"] * 3 + ["pedestrian"] * 3 + ["animal"] * 3
        n_inside = [int(v) for v in rng.permutation(np.arange(G) % 11)]
        boxes, points, cells, used = scene(rng, names, n_inside, n_points - sum(n_inside), far=((0, (50.5, 50.0)), (1, (56.0, 0.0))))

        def where(cls, k, rng=rng, boxes=boxes):
            if k % 3 == 0:                                    # on top of a ground-truth row or of another candidate
                b = boxes[int(rng.integers(0, len(boxes) - 2))]
                return b[0] + rng.uniform(-1, 1), b[1] + rng.uniform(-1, 1)
            return rng.uniform(-44, 44), rng.uniform(-44, 44)
        order = ["car", "truck", "pedestrian"]
        have = {c: sum(1 for g in range(G) if names[g] == c and (min_points <= 0 or n_inside[g] >= min_points)) for c in order}
        db = database(rng, {c: n_draw[i] + 6 for i, c in enumerate(order)}, where)
        groups = [{c: have[c] + n_draw[i]} for i, c in enumerate(order)]
        try:
            flat, out = drive(mods, tmp, name, sd, points, boxes, names, db, groups, min_points, (-0.3925, 0.3925), (0.95, 1.05), std)
            assert tuple(out["global"][:2]) == tuple(float(v) for v in want_flips), "flips"
            assert len(out["cand_boxes"]) == sum(n_draw) and 0 < out["accept"].sum() < len(out["accept"]), "accept"
            assert (~out["range_mask"]).any() and out["range_mask"].sum() >= 3, "range"
            if min_points > 0:
                assert (out["keep"] == 0).any()
        except AssertionError as e:
            print(name, "seed", sd, "refused:", e)
            continue
        print(name, "seed", sd, "counts", out["counts"].tolist(), "accept", out["accept"].tolist(), "global", out["global"].round(3).tolist(),
              "in range", int(out["range_mask"].sum()), "of", len(out["range_mask"]))
        flat[name + "_seed"] = np.int32(sd)
        return flat
    raise SystemExit("no seed for " + name)


def case_order(mods, tmp):
    """the planted select cases; boxes 2 m x 2 m along the x axis, heading 0.  Group 0 (car), in draw order: the mutual pair a0, a1; the
    chain c0 - c1 - c2; d on a ground-truth row that keep dropped; e, free; h on a kept ground-truth row.  Group 1 (pedestrian): p on the
    accepted e; q on the rejected a0 only; f, free."""
    rng = np.random.default_rng(5)

    def box(x):
        # (y differs from box to box: two axis-aligned squares with the same y extent have no properly crossing edges)
        return np.array([x, 0.3 * np.cos(3.0 * x), -1.0, 2.0, 2.0, 1.6, 1.0, -2.0, 0.0], np.float32)
    gt = np.stack([box(-10.0), box(20.0)])
    names = ["car", "car"]
    points = np.concatenate([inner_points(rng, gt[0], 3), np.stack([rng.uniform(-40, 40, 200), rng.uniform(5, 40, 200), rng.uniform(1.5, 3, 200),
                                                                    rng.uniform(0, 1, 200), rng.uniform(0, 0.5, 200)], 1).astype(np.float32)], 0)
    cars = [0.0, 1.5, 10.0, 11.5, 13.0, 20.3, 30.0, -10.5]
    peds = [30.5, -0.9, 44.0]

    def infos(cls, xs):
        return [dict(name=cls, box3d_lidar=box(x), points=inner_points(rng, np.array([0, 0, 0, 2, 2, 1.6, 0, 0, 0], np.float32), 4 + k), difficulty=0)
                for k, x in enumerate(xs)]
    db = dict(car=infos("car", cars + [90.0, 95.0]), pedestrian=infos("pedestrian", peds + [90.0, 95.0]))
    groups = [{"car": 1 + len(cars)}, {"pedestrian": len(peds)}]      # one car of the ground truth is left after the min-points mask
    for sd in range(1, 200):
        try:
            flat, out = drive(mods, tmp, "order", sd, points, gt, names, db_copy(db), groups, 1, (-0.3925, 0.3925), (0.95, 1.05), 0.0, keep_order=True)
        except AssertionError as e:
            print("order seed", sd, "refused:", e)
            continue
        break
    assert out["keep"].tolist() == [1, 0] and out["cand_group"].tolist() == [0] * 8 + [1] * 3
    #                               a0 a1 c0 c1 c2 d  e  h  p  q  f
    assert out["accept"].tolist() == [0, 1, 0, 0, 1, 1, 1, 0, 0, 1, 1], out["accept"].tolist()
    print("order accept", out["accept"].tolist())
    return flat


def db_copy(db):
    return {k: [dict(i, box3d_lidar=i["box3d_lidar"].copy(), points=i["points"].copy()) for i in v] for k, v in db.items()}


def case_plants(mods, tmp):
    """points on a box face and its fp32 neighbours (x, y and z faces of an axis-aligned box whose faces are fp32 numbers); rows whose
    best BEV corner is on the range edge, a row that straddles it, a row outside; no rotation, scale 1, no translation, no candidates"""
    f = np.float32
    gt = np.array([[10.0, 4.0, -1.0, 2.0, 4.0, 1.5, 0.5, 0.25, 0.0],
                   [-20.0, -8.0, -1.0, 1.0, 1.0, 2.0, 0.0, 0.0, 0.0],
                   [52.2, 0.0, -1.0, 2.0, 2.0, 1.5, 0.0, 0.0, 0.0],            # its inner corners at x = 51.2 up to the rounding of 52.2
                   [51.2, 10.0, -1.0, 2.0, 2.0, 1.5, 0.0, 0.0, 0.0],           # straddles: kept
                   [0.0, -52.2, -1.0, 2.0, 2.0, 1.5, 0.0, 0.0, 0.0],           # inner corners at y = -51.2
                   [30.0, 60.0, -1.0, 2.0, 2.0, 1.5, 0.0, 0.0, 0.0]], f)        # outside
    names = ["car", "pedestrian", "car", "truck", "car", "car"]
    rng = np.random.default_rng(9)
    face = []
    for base in ((f(11.0), f(4.5), f(-1.0)), (f(10.5), f(6.0), f(-1.0)), (f(10.5), f(4.5), f(-0.25))):       # x, y, z faces of row 0
        for axis in range(3):
            if base[axis] in (f(11.0), f(6.0), f(-0.25)):
                for v in (np.nextafter(base[axis], f(-100)), base[axis], np.nextafter(base[axis], f(100))):
                    p = list(base)
                    p[axis] = v
                    face.append(p + [0.5, 0.1])
    face = np.array(face, f)
    assert len(face) == 9
    inner = np.concatenate([inner_points(rng, gt[g], 3) for g in range(6)], 0)
    bg = np.stack([rng.uniform(-51, 51, 300), rng.uniform(-51, 51, 300), rng.uniform(1.5, 3, 300), rng.uniform(0, 1, 300), rng.uniform(0, 0.5, 300)], 1)
    points = np.concatenate([face, inner, bg.astype(f)], 0)
    plants = dict(pairs=[(i, 0) for i in range(9)], range_rows=[2, 4])
    for sd in range(1, 200):
        flat, out = drive(mods, tmp, "plants", sd, points, gt, names, None, None, 3, (0.0, 0.0), (1.0, 1.0), 0.0, plants=plants)
        if tuple(out["global"][:2]) == (0.0, 0.0):
            break
    assert out["global"].tolist() == [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    flat["plants_face_points"] = np.int32(9)
    flat["plants_range_rows"] = np.array([2, 4], np.int32)
    print("plants counts", out["counts"].tolist(), "range", out["range_mask"].tolist())
    return flat


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    mods = reference_modules(sys.argv[1])
    z = {}
    with tempfile.TemporaryDirectory() as tmp:
        z.update(case_scene(mods, tmp, "nusc", 100, 14, (5, 4, 3), 3000, (1, 1), 5, 0.2))
        for k, fl in enumerate(((0, 0), (1, 0), (0, 1))):
            z.update(case_scene(mods, tmp, f"flips{k}", 200 + 100 * k, 6, (2, 1, 1), 400, fl, -1, 0.0))
        z.update(case_order(mods, tmp))
        z.update(case_plants(mods, tmp))
    z["cases"] = np.array(["nusc", "flips0", "flips1", "flips2", "order", "plants"])
    z["class_names"] = np.array(CLASS_NAMES)
    z["numpy_version"] = np.array(np.__version__)
    out = os.path.join(HERE, "cp_augment_vectors.npz")
    np.savez_compressed(out, **z)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 1000 * 1000


if __name__ == "__main__":
    main()
