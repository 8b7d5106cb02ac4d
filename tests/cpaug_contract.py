"""The four md_cp_aug_* operators (include/minddet_hip_cpaug.h) restated in numpy float64, one sample at a time, with the margin of every
point-in-box and corner-in-range decision and with forward bounds of the reference's fp32 operation sequence.  The collision predicate
and the rectangle are those of tests/pcaug_contract.py (collide, rect), imported, not restated.

Decisions.  A point is inside a box iff s = min(w/2 - |lx|, l/2 - |ly|, h/2 - |dz|) > 0 (the box frame is centred in z); |s| is the
distance to the nearest face, the decision's margin.  A BEV corner is inside the range iff s = min(x - xmin, xmax - x, y - ymin,
ymax - y) > 0; a box is kept iff its largest s is > 0.  A decision is DECIDED when its margin exceeds MARGIN = 5e-4 m.

MARGIN, derived for nuScenes extents (points and boxes within +-61 m on both axes, boxes up to about 15 m), u = 2^-24 = 6e-8:
  * the reference forms the eight corners in fp32 (center_to_corner_box3d): a corner coordinate is up to R = 61 sqrt(2) + 7.5 = 94 m,
    one rounding is u R = 5.6e-6 m, and a coordinate passes four (two products and a sum of the rotation, the centre added): 2.2e-5 m,
    3e-5 m as a displacement of the corner.  That moves a face's plane by up to 3e-5 m and tilts it by up to 2 x 3e-5 m over the
    length of the edge the normal was formed from, i.e. by another 6e-5 m anywhere on the face: 9e-5 m.
  * the sign expression p . n + d (geometry.py, surface_equ_3d_jitv2 and _points_count_convex_polygon_3d_jit) is evaluated in fp32
    with terms up to R |n| for p . n and the same for d = -n . corner: three products and three sums each, at most 8 u R |n| in all,
    which divided by |n| is 4.5e-5 m.
  Sum 1.4e-4 m; MARGIN is about four times that.  A corner against the range edge has only the first item (3e-5 m).
The collision decisions carry no margin: the fixture's generator asserts that box_collision_test on the reference's fp32 corners and
this module's predicate on float64 corners agree on every pair it looks at.

Bounds.  u = 2^-24.  The reference keeps boxes and points in fp32 and rounds after every step.  Adding the box centre to a candidate's
points: u |result|.  A flip is exact for a coordinate; r -> -r + pi (2 pi) takes pi in fp32 and rounds: u (pi + |r|), u (2 pi + |r|).
A rotation x c + y s with c, s stored in fp32 costs at most 4 u (|x| + |y|) and carries an earlier error e on as at most sqrt(2) e (the
velocities are rotated in float64 and rounded once, which the same expression covers); r += rot takes rot in fp32: u (|rot| + |r|).
The scale is taken in fp32 and the product rounded: 2 u |result| on top of |scale| e.  The translation is added in float64 and rounded:
u |result|.  Every bound adds u |result| for the operator's own single rounding.
"""
import numpy as np

from tests.pcaug_contract import collide, rect

MARGIN = 5e-4
U = 2.0 ** -24


def signed_inside(points, boxes):
    """[N, K] signed distance to the nearest face, positive inside (float64); boxes [K, 9], centred in z"""
    p, q = points.astype(np.float64), boxes.astype(np.float64)
    dx, dy, dz = (p[:, None, k] - q[None, :, k] for k in range(3))
    c, s = np.cos(q[:, 8])[None], np.sin(q[:, 8])[None]
    lx, ly = dx * c - dy * s, dx * s + dy * c
    return np.minimum(np.minimum(q[None, :, 3] / 2 - np.abs(lx), q[None, :, 4] / 2 - np.abs(ly)), q[None, :, 5] / 2 - np.abs(dz))


def count_points(points, gt_boxes, count, min_points):
    """one sample -> dict: counts [G] i32, keep [G] u8, lo / hi [G] (the count with every undecided pair out / in), keep_decided [G],
    margin [N, count], decided (every pair decided)"""
    G = len(gt_boxes)
    s = signed_inside(points, gt_boxes[:count]) if count else np.zeros((len(points), 0))
    counts, lo, hi = np.zeros(G, np.int32), np.zeros(G, np.int64), np.zeros(G, np.int64)
    counts[:count] = (s > 0).sum(0)
    lo[:count] = (s > MARGIN).sum(0)
    hi[:count] = lo[:count] + (np.abs(s) <= MARGIN).sum(0)
    below = np.arange(G) < count
    keep = below & ((min_points <= 0) | (counts >= min_points))
    keep_decided = ~below | (min_points <= 0) | (lo >= min_points) | (hi < min_points)
    return dict(counts=counts, keep=keep.astype(np.uint8), lo=lo, hi=hi, keep_decided=keep_decided, margin=np.abs(s),
                decided=bool((np.abs(s) > MARGIN).all()))


def bev_corners(boxes):
    """[K, 9] -> x [K, 4], y [K, 4]: center_to_corner_box2d(xy, wl, r) in float64"""
    b = boxes.astype(np.float64).reshape(-1, 9)
    x, y = rect(b[:, 3], b[:, 4], b[:, 8])
    return x + b[:, 0:1], y + b[:, 1:2]


def collision_matrix(boxes):
    """box_collision_test(total_bv, total_bv): [K, K] bool, row = first argument"""
    x, y = bev_corners(boxes)
    return collide(x[:, None, :], y[:, None, :], x[None], y[None])[3]


def select(gt_boxes, count, keep, cand_boxes, cand_count, cand_group):
    """one sample, the literal loop of sample_all / sample_class_v2 -> accept [S] u8.  A decreasing group: nothing accepted."""
    S = len(cand_boxes)
    accept = np.zeros(S, np.uint8)
    grp = np.asarray(cand_group[:cand_count])
    if cand_count == 0 or (np.diff(grp) < 0).any():
        return accept
    avoid = gt_boxes[:count][np.asarray(keep[:count]) != 0]
    i = 0
    while i < cand_count:
        e = i + 1
        while e < cand_count and grp[e] == grp[i]:
            e += 1
        sp = cand_boxes[i:e]
        num_gt, num_sampled = len(avoid), len(sp)
        coll = collision_matrix(np.concatenate([avoid.reshape(-1, 9), sp], 0))
        coll[np.arange(len(coll)), np.arange(len(coll))] = False
        valid = []
        for k in range(num_gt, num_gt + num_sampled):
            if coll[k].any():
                coll[k] = False
                coll[:, k] = False
            else:
                valid.append(k - num_gt)
        accept[i + np.array(valid, np.int64)] = 1
        avoid = np.concatenate([avoid.reshape(-1, 9), sp[valid]], 0)
        i = e
    return accept


def _rot(x, y, ang):
    c, s = np.cos(ang), np.sin(ang)
    return x * c + y * s, -x * s + y * c


def augment_points(points, glob, cand_points=None, cand_offsets=None, cand_boxes=None, accept=None):
    """one sample (cand_offsets [S + 1] into cand_points) -> dict: points [n, F] f32 (the accepted candidates' points, then the scene's),
    exact [n, 3] f64, bound [n] (forward bound of the reference's fp32 sequence, max-norm over x, y, z), n_cand (rows from candidates)"""
    F = points.shape[1]
    parts, errs = [], []
    if cand_points is not None:
        for s in np.flatnonzero(np.asarray(accept) != 0):
            p = cand_points[cand_offsets[s]:cand_offsets[s + 1]].astype(np.float64)
            p[:, :3] += cand_boxes[s, :3].astype(np.float64)
            parts.append((p, cand_points[cand_offsets[s]:cand_offsets[s + 1]]))
            errs.append(U * np.abs(p[:, :3]).max(1))
    n_cand = sum(len(p) for p, _ in parts)
    parts.append((points.astype(np.float64), points))
    errs.append(np.zeros(len(points)))
    p = np.concatenate([a for a, _ in parts], 0)
    raw = np.concatenate([b for _, b in parts], 0)
    e = np.concatenate(errs)
    x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    if glob[0] != 0:
        y = -y
    if glob[1] != 0:
        x = -x
    e = np.sqrt(2) * e + 4 * U * (np.abs(x) + np.abs(y))
    x, y = _rot(x, y, glob[2])
    s = glob[3]
    x, y, z = x * s, y * s, z * s
    big = lambda: np.maximum(np.maximum(np.abs(x), np.abs(y)), np.abs(z))   # noqa: E731
    e = abs(s) * e + 2 * U * big()
    x, y, z = x + glob[4], y + glob[5], z + glob[6]
    e = e + 2 * U * big()                                                   # the translation's rounding and the operator's own
    out = np.zeros((len(p), F), np.float32)
    out[:, 0], out[:, 1], out[:, 2] = x.astype(np.float32), y.astype(np.float32), z.astype(np.float32)
    out[:, 3:] = raw[:, 3:]
    return dict(points=out, exact=np.stack([x, y, z], 1), bound=e, n_cand=n_cand)


def augment_boxes(gt_boxes, gt_classes, count, keep, glob, bv_range, cand_boxes=None, cand_classes=None, accept=None):
    """one sample -> dict: gt_boxes [G+S, 9] f32 and gt_classes [G+S] i32 (compacted, zero rows behind), count, sel [G+S] bool (the
    selected input rows: ground truth then candidates), all [n_sel, 9] f64 (every selected row transformed), mask [n_sel] (the range
    decision), margin [n_sel], bound [n_sel, 9] (forward bound per element)"""
    G = len(gt_boxes)
    S = 0 if cand_boxes is None else len(cand_boxes)
    rows = gt_boxes if S == 0 else np.concatenate([gt_boxes, cand_boxes], 0)
    cls = np.asarray(gt_classes, np.int32) if S == 0 else np.concatenate([np.asarray(gt_classes, np.int32), np.asarray(cand_classes, np.int32)])
    sel = np.zeros(G + S, bool)
    sel[:G] = (np.arange(G) < count) & (np.asarray(keep) != 0) & (cls[:G] > 0)
    if S:
        sel[G:] = (np.asarray(accept) != 0) & (cls[G:] > 0)
    b = rows[sel].astype(np.float64).reshape(-1, 9)
    n = len(b)
    x, y, z, w, l, h, vx, vy, r = (b[:, k].copy() for k in range(9))
    e = np.zeros((n, 9))
    if glob[0] != 0:
        y, vy, r = -y, -vy, -r + np.pi
        e[:, 8] += U * (np.pi + np.abs(r))
    if glob[1] != 0:
        x, vx, r = -x, -vx, -r + 2 * np.pi
        e[:, 8] += U * (2 * np.pi + np.abs(r))
    e[:, 0] = e[:, 1] = 4 * U * (np.abs(x) + np.abs(y))
    e[:, 6] = e[:, 7] = 4 * U * (np.abs(vx) + np.abs(vy))
    x, y = _rot(x, y, glob[2])
    vx, vy = _rot(vx, vy, glob[2])
    r = r + glob[2]
    e[:, 8] += U * (abs(glob[2]) + np.abs(r))
    s = glob[3]
    x, y, z, w, l, h, vx, vy = (v * s for v in (x, y, z, w, l, h, vx, vy))
    e[:, :8] = abs(s) * e[:, :8] + 2 * U * np.abs(np.stack([x, y, z, w, l, h, vx, vy], 1))
    x, y, z = x + glob[4], y + glob[5], z + glob[6]
    e[:, :3] += U * np.abs(np.stack([x, y, z], 1))
    cx, cy = rect(w, l, r)
    cx, cy = cx + x[:, None], cy + y[:, None]
    sd = np.minimum(np.minimum(cx - bv_range[0], bv_range[2] - cx), np.minimum(cy - bv_range[1], bv_range[3] - cy))
    mask = (sd > 0).any(1) if n else np.zeros(0, bool)
    margin = np.abs(sd.max(1)) if n else np.zeros(0)      # the decision flips where the largest signed distance crosses zero
    allb = np.stack([x, y, z, w, l, h, vx, vy, r], 1) if n else np.zeros((0, 9))
    e += U * np.abs(allb)                                  # the operator's own rounding
    out, out_cls = np.zeros((G + S, 9), np.float32), np.zeros(G + S, np.int32)
    k = int(mask.sum())
    out[:k], out_cls[:k] = allb[mask].astype(np.float32), cls[sel][mask]
    return dict(gt_boxes=out, gt_classes=out_cls, count=k, sel=sel, all=allb, mask=mask, margin=margin, bound=e)
