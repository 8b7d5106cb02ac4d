"""Golden vectors for the point-cloud augmentation, produced BY THE REFERENCE: the training branch of prep_pointcloud
(minddet/models/pointpillars/src/data/preprocess.py:124-170) driven step by step with the reference's own routines of
src/core/preprocess.py (remove_points_in_boxes, noise_per_object, random_flip, global_rotation, global_scaling, global_translate,
filter_gt_box_outside_range) and box_np_ops.limit_period.  numpy's generator is seeded and np.random.normal / uniform / choice are
wrapped during the calls, so the float64 draws the reference used are recorded and become the operators' inputs.  Run here only:

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/gen_pc_augment.py

Asserted while generating: (i) noise_per_box[_v2_] run a second time on float64 boxes selects the same tries; (ii) in no pair that
box_collision_test looks at does _get_box_overlap_another hold while _get_ret does not (quirk (a) of include/minddet_hip_pcaug.h: the
identity comparison skips the containment tests under the shim; on the fixture both readings coincide).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True
from gen_golden import _shim  # noqa: E402

BV_RANGE = np.array([0, -39.68, 69.12, 39.68], np.float32)


def to_lidar(local, box):
    """points given in a box's frame (x along w, y along l, z up from the bottom) -> lidar, float64"""
    c, s = np.cos(np.float64(box[6])), np.sin(np.float64(box[6]))
    x = local[:, 0] * c + local[:, 1] * s + np.float64(box[0])
    y = -local[:, 0] * s + local[:, 1] * c + np.float64(box[1])
    return np.stack([x, y, local[:, 2] + np.float64(box[2])], 1)


def scene(rng, G, sizes, n_points, plants):
    boxes = np.zeros((G, 7), np.float32)
    # spread on a jittered grid so that the originals do not overlap (the planted pair aside)
    cells = [(x, y) for x in np.arange(8, 64, 8.0) for y in np.arange(-30, 31, 10.0)]
    pick = rng.permutation(len(cells))[:G]
    for g, k in enumerate(pick):
        w, l = sizes[g % len(sizes)]
        boxes[g] = (cells[k][0] + rng.uniform(-1, 1), cells[k][1] + rng.uniform(-1, 1), rng.uniform(-1.8, -1.2), w, l, rng.uniform(1.4, 1.8),
                    rng.uniform(-np.pi, np.pi))
    # two boxes that straddle the range edge before the global steps
    boxes[G - 1, :2] = (68.9, rng.uniform(-20, 20))
    boxes[G - 2, :2] = (rng.uniform(20, 50), 39.5)
    n_in = n_points // 2
    pts = []
    for k in range(n_in):
        b = boxes[k % G]
        loc = np.array([[rng.uniform(-0.49, 0.49) * b[3], rng.uniform(-0.49, 0.49) * b[4], rng.uniform(0.01, 0.99) * b[5]]])
        pts.append(to_lidar(loc, b)[0])
    for k in range(plants):                                   # on a face: w / 2 exactly, before the rounding to fp32
        b = boxes[k % G]
        loc = np.array([[0.5 * np.float64(b[3]), rng.uniform(-0.4, 0.4) * b[4], 0.5 * b[5]]])
        pts.append(to_lidar(loc, b)[0])
    pts = np.array(pts)
    bg = np.stack([rng.uniform(0, 69, n_points - len(pts)), rng.uniform(-39, 39, n_points - len(pts)), rng.uniform(-2.5, 0.5, n_points - len(pts))], 1)
    xyz = np.concatenate([pts, bg])[rng.permutation(n_points)]
    points = np.concatenate([xyz, rng.uniform(0, 1, (n_points, 1))], 1).astype(np.float32)
    return boxes, points


class Capture:
    """np.random.normal / uniform / choice wrapped: every draw recorded (the returned object itself, which the reference may modify in
    place, and a copy taken at the draw); `edit` may change an array draw before the reference sees it"""

    def __init__(self, edit=None):
        self.draws, self.edit = [], edit

    def __enter__(self):
        self.saved = (np.random.normal, np.random.uniform, np.random.choice)

        def wrap(kind, fn):
            def inner(*a, **k):
                v = fn(*a, **k)
                if self.edit is not None and isinstance(v, np.ndarray) and v.ndim >= 2:
                    self.edit(kind, len(self.draws), v)
                self.draws.append((kind, v, np.array(v, copy=True)))
                return v
            return inner

        np.random.normal, np.random.uniform, np.random.choice = (wrap(k, f) for k, f in zip(("normal", "uniform", "choice"), self.saved))
        return self

    def __exit__(self, *exc):
        np.random.normal, np.random.uniform, np.random.choice = self.saved


def run_case(prep, box_np_ops, name, seed, G, sizes, n_points, plants, grot_range, invalid, zero_rows=(), overlap=None, n_remove=0,
             n_front=0, T=100, rot_perturb=(-0.15707963267, 0.15707963267), loc_std=(0.25, 0.25, 0.25)):
    rng = np.random.default_rng(seed)
    np.random.seed(seed)
    gt_boxes, bg = scene(rng, G, sizes, n_points - n_front, plants)
    if overlap is not None:                                    # box overlap[1] on top of box overlap[0], slightly moved and turned
        gt_boxes[overlap[1]] = gt_boxes[overlap[0]]
        gt_boxes[overlap[1], :2] += (0.4, 0.3)
        gt_boxes[overlap[1], 6] += 0.3
    valid = np.ones(G, np.bool_)
    valid[list(invalid)] = False
    classes = (1 + np.arange(G) % 2).astype(np.int32)
    out = {}
    remove_boxes = np.zeros((0, 7), np.float32)
    front = np.zeros((0, 4), np.float32)
    points = bg
    if n_remove:
        # the sampler's result: boxes dropped into the scene with their own points in front (data/preprocess.py:110-127)
        remove_boxes = np.zeros((n_remove, 7), np.float32)
        for r in range(n_remove):
            remove_boxes[r] = (rng.uniform(10, 60), rng.uniform(-30, 30), -1.5, 6.0, 9.0, 1.7, rng.uniform(-3, 3))
        per = n_front // n_remove
        front = np.concatenate([np.concatenate([to_lidar(np.stack([rng.uniform(-0.45, 0.45, per) * 6.0, rng.uniform(-0.45, 0.45, per) * 9.0,
                                                                   rng.uniform(0.1, 1.6, per)], 1), remove_boxes[r]),
                                                rng.uniform(0, 1, (per, 1))], 1) for r in range(n_remove)]).astype(np.float32)
        n_front = len(front)
        kept = prep.remove_points_in_boxes(bg, remove_boxes)
        masks = box_np_ops.points_in_rbbox(bg, remove_boxes)
        out["removed"] = masks.any(-1)
        assert len(kept) == int((~out["removed"]).sum()) and out["removed"].any()
        points = np.concatenate([front, kept], 0)
    out.update(gt_boxes=gt_boxes.copy(), valid=valid.astype(np.uint8), classes=classes, points=np.concatenate([front, bg], 0),
               remove_boxes=remove_boxes, remove_from=np.int32(n_front), bv_range=BV_RANGE)

    record = {}
    real = dict(v1=prep.noise_per_box, v2=prep.noise_per_box_v2_, coll=prep.box_collision_test, mask=prep.points_in_convex_polygon_3d_jit)

    def selecting(which):
        def inner(boxes, valid_mask, loc, rot, *grot):
            again = real[which](boxes.astype(np.float64), valid_mask, loc.copy(), rot.copy(), *[g.copy() for g in grot])
            sel = real[which](boxes, valid_mask, loc, rot, *grot)
            assert np.array_equal(sel, again), f"{name}: fp32 and float64 boxes select different tries, pick another seed"   # (i)
            record["selected"] = np.array(sel)
            return sel
        return inner

    def colliding(boxes, qboxes, clockwise=True):
        ret = real["coll"](boxes, qboxes, clockwise)
        slices = np.array([1, 2, 3, 0])
        lb, lq = np.stack((boxes, boxes[:, slices, :]), axis=2), np.stack((qboxes, qboxes[:, slices, :]), axis=2)
        sb, sq = box_np_ops.corner_to_standup_nd_jit(boxes), box_np_ops.corner_to_standup_nd_jit(qboxes)
        for i in range(boxes.shape[0]):
            for j in range(qboxes.shape[0]):
                if min(sb[i, 2], sq[j, 2]) - max(sb[i, 0], sq[j, 0]) > 0 and min(sb[i, 3], sq[j, 3]) - max(sb[i, 1], sq[j, 1]) > 0:
                    edges = prep._get_ret(lb, lq, i, j)
                    over = prep._get_box_overlap_another(boxes, qboxes, clockwise, i, j) or \
                        prep._get_box_overlap_another(qboxes, boxes, clockwise, j, i)
                    assert edges or not over, f"{name}: containment without crossing edges, the two readings of quirk (a) differ"   # (ii)
                    assert bool(ret[i, j]) == bool(edges)
        return ret

    def masking(pts, surfaces, *a):
        m = real["mask"](pts, surfaces, *a)
        record["point_masks"] = np.array(m)
        return m

    def edit(kind, index, v):
        for g in zero_rows:
            v[g] = 0.0

    prep.noise_per_box, prep.noise_per_box_v2_ = selecting("v1"), selecting("v2")
    prep.box_collision_test, prep.points_in_convex_polygon_3d_jit = colliding, masking
    boxes, pts = gt_boxes.copy(), points.copy()
    try:
        with Capture(edit) as cap:
            prep.noise_per_object(boxes, pts, valid, rotation_perturb=list(rot_perturb), center_noise_std=list(loc_std),
                                  global_random_rot_range=list(grot_range), num_try=T)
    finally:
        prep.noise_per_box, prep.noise_per_box_v2_ = real["v1"], real["v2"]
        prep.box_collision_test, prep.points_in_convex_polygon_3d_jit = real["coll"], real["mask"]
    (k0, loc_after, loc), (k1, rot_after, rot), (k2, _, grot) = cap.draws
    assert (k0, k1, k2) == ("normal", "uniform", "uniform") and loc.shape == (G, T, 3) and rot.shape == grot.shape == (G, T)
    enable_grot = abs(grot_range[0] - grot_range[1]) >= 1e-3
    sel = record["selected"]
    tf = np.zeros((G, 4))
    for g in range(G):
        if sel[g] >= 0:
            tf[g, :3], tf[g, 3] = loc_after[g, sel[g]], rot_after[g, sel[g]]
    out.update(loc=loc, rot=rot, selected=sel.astype(np.int32), obj_transform=tf, point_masks=record["point_masks"],
               boxes_noise=boxes.copy(), points_noise=pts.copy(), enable_grot=np.bool_(enable_grot))
    if enable_grot:
        out["grot"] = grot
    boxes_v, cls_v = boxes[valid], classes[valid]
    with Capture() as cap:
        boxes_v, pts = prep.random_flip(boxes_v, pts)
        out.update(boxes_flip=boxes_v.copy(), points_flip=pts.copy())
        boxes_v, pts = prep.global_rotation(boxes_v, pts, rotation=[-0.78539816, 0.78539816])
        out.update(boxes_rot=boxes_v.copy(), points_rot=pts.copy())
        boxes_v, pts = prep.global_scaling(boxes_v, pts, 0.95, 1.05)
        out.update(boxes_scale=boxes_v.copy(), points_scale=pts.copy())
        boxes_v, pts = prep.global_translate(boxes_v, pts, (0.2, 0.2, 0.2))
        out.update(boxes_translate=boxes_v.copy(), points_translate=pts.copy())
    vals = [float(np.asarray(c).reshape(-1)[0]) for _, _, c in cap.draws]
    assert [k for k, _, _ in cap.draws] == ["choice", "uniform", "uniform", "normal", "normal", "normal"]
    out["global"] = np.array(vals, np.float64)
    mask = prep.filter_gt_box_outside_range(boxes_v, BV_RANGE)
    final = boxes_v[mask]
    final[:, 6] = box_np_ops.limit_period(final[:, 6], offset=0.5, period=2 * np.pi)
    out.update(range_mask=mask, final_boxes=final, final_classes=cls_v[mask])
    assert boxes.dtype == pts.dtype == final.dtype == np.float32
    return {f"{name}_{k}": v for k, v in out.items()}


def collision_case(prep, box_np_ops, rng):
    """40 planted pairs (A, B as x, y, w, l, r): crossing edges, A inside B, B inside A, apart inside the standup overlap, far apart"""
    A, Bq = np.zeros((40, 5), np.float32), np.zeros((40, 5), np.float32)
    for k in range(40):
        kind = k % 5
        cx, cy = rng.uniform(5, 60), rng.uniform(-30, 30)
        Bq[k] = (cx, cy, rng.uniform(1.5, 2.0), rng.uniform(3.5, 4.5), rng.uniform(-3, 3))
        if kind == 0:
            A[k] = (cx + rng.uniform(0.3, 0.8), cy + rng.uniform(-0.5, 0.5), 1.8, 4.0, Bq[k, 4] + rng.uniform(0.6, 1.0))
        elif kind == 1:
            A[k] = (cx + rng.uniform(-0.1, 0.1), cy + rng.uniform(-0.1, 0.1), 0.6, 0.8, rng.uniform(-3, 3))
        elif kind == 2:
            A[k] = (cx + rng.uniform(-0.1, 0.1), cy + rng.uniform(-0.1, 0.1), 8.0, 9.0, rng.uniform(-3, 3))
        elif kind == 3:
            Bq[k, 4] = np.pi / 4                                # two long thin boxes side by side on a diagonal: bounds overlap, boxes do not
            Bq[k, 2:4] = (0.6, 6.0)
            A[k] = (cx + 1.2, cy - 1.2, 0.6, 6.0, np.pi / 4)
        else:
            A[k] = (cx + 12.0, cy, 1.8, 4.0, rng.uniform(-3, 3))
    ca, cb = box_np_ops.box2d_to_corner_jit(A), box_np_ops.box2d_to_corner_jit(Bq)
    sl = np.array([1, 2, 3, 0])
    la, lb = np.stack((ca, ca[:, sl, :]), axis=2), np.stack((cb, cb[:, sl, :]), axis=2)
    sa, sb = box_np_ops.corner_to_standup_nd_jit(ca), box_np_ops.corner_to_standup_nd_jit(cb)
    edges = np.array([prep._get_ret(la, lb, k, k) for k in range(40)])
    a_b = np.array([prep._get_box_overlap_another(ca, cb, True, k, k) for k in range(40)])
    b_a = np.array([prep._get_box_overlap_another(cb, ca, True, k, k) for k in range(40)])
    standup = np.array([min(sa[k, 2], sb[k, 2]) - max(sa[k, 0], sb[k, 0]) > 0 and min(sa[k, 3], sb[k, 3]) - max(sa[k, 1], sb[k, 1]) > 0
                        for k in range(40)])
    assert edges[0::5].all(), "crossing pairs"
    assert b_a[1::5].all() and not a_b[1::5].any() and not edges[1::5].any(), "A inside B"
    assert a_b[2::5].all() and not b_a[2::5].any() and not edges[2::5].any(), "B inside A"
    assert standup[3::5].all() and not (edges | a_b | b_a)[3::5].any(), "apart inside the standup overlap"
    assert not standup[4::5].any(), "far apart"
    return dict(collision_a=A, collision_b=Bq, collision_edges=edges, collision_a_covers_b=a_b, collision_b_covers_a=b_a,
                collision_standup=standup)


def main():
    _shim()
    from src.core import box_np_ops  # the reference's own modules
    from src.core import preprocess as prep

    from tests import pcaug_contract as pc

    car, ped, cyc = (1.6, 3.9), (0.6, 0.8), (0.6, 1.76)
    z = {}

    def capped(name, case):
        """the condition of tests/test_pc_augment_cpu.py on the scene: undecided pairs, plants included, <= 2e-3 of the pairs within 1 m"""
        f = {k[len(name) + 1:]: v for k, v in case.items()}
        G, R = len(f["gt_boxes"]), len(f["remove_boxes"])
        p = pc.augment_points(f["points"], f["gt_boxes"], G, f["valid"], f["obj_transform"], f["global"], f["remove_boxes"] if R else None, R,
                              int(f["remove_from"]))
        undecided, near = int((p["margin"] <= pc.MARGIN).sum()), int(p["near"].sum())
        assert 1 <= undecided <= 2e-3 * near, f"{name}: {undecided} undecided of {near} pairs within 1 m of a face"
        print(name, "undecided", undecided, "of", near, "near pairs")

    def first_seed(name, start, *args, **kw):
        for seed in range(start, start + 50):                  # "pick another seed": the first one on which every assertion holds
            try:
                case = run_case(prep, box_np_ops, name, seed, *args, **kw)
                capped(name, case)
            except AssertionError as e:
                print(name, "seed", seed, "refused:", e)
                continue
            z.update(case)
            z[name + "_seed"] = np.int32(seed)
            return
        raise SystemExit("no seed for " + name)

    # plants: few enough for the cap (2 of about 1 400 near pairs, 1 of about 700), present in every case
    first_seed("car", 11, 12, [car], 3000, 2, (0.78, 2.35), invalid=[5], zero_rows=(0, 7), overlap=(0, 7))
    first_seed("nogrot", 12, 12, [car], 1500, 1, (0.0, 0.0), invalid=[3])
    first_seed("pedcyc", 13, 20, [ped, cyc, car, (1.9, 4.6)], 1500, 1, (0.78, 2.35), invalid=[2, 9], n_remove=3, n_front=240,
               rot_perturb=(-np.pi / 3, np.pi / 3), loc_std=(1.0, 1.0, 1.0))
    z.update(collision_case(prep, box_np_ops, np.random.default_rng(14)))
    flips = [z[f"{c}_global"][0] for c in ("car", "nogrot", "pedcyc")]
    assert 0.0 in flips and 1.0 in flips, flips
    assert z["car_selected"][0] == -1 and z["car_selected"][7] == -1 and (z["car_selected"][[1, 2, 3, 4, 6]] >= 0).all()
    for c in ("car", "nogrot", "pedcyc"):
        m = z[f"{c}_range_mask"]
        print(c, "selected", z[f"{c}_selected"].tolist(), "flip", z[f"{c}_global"][0], "in range", int(m.sum()), "of", len(m))
    z["cases"] = np.array(["car", "nogrot", "pedcyc"])
    z["numpy_version"] = np.array(np.__version__)
    out = os.path.join(HERE, "pc_augment_vectors.npz")
    np.savez_compressed(out, **z)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 1000 * 1000


if __name__ == "__main__":
    main()
