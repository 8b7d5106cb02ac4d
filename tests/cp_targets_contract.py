"""The contract of md_cp_assign_targets (include/minddet_hip_cptargets.h) as vectorised numpy: membership and slots, the wrapped heading,
sizes and centres in cells, the Gaussian radius, the heat maps, the rows and gt_boxes_and_cls -- with the header's number formats (fp32
array arithmetic for the geometry, the Gaussian in float64 rounded to fp32 by the window maximum).  No Python loop over cells; one over
the drawn objects.  tests/test_cp_targets_cpu.py shows it equals the reference's own outputs (tests/golden/cp_target_vectors.npz);
tests/test_cp_targets_gpu.py uses it for shapes the fixture does not carry.  The accuracy conditions both tests apply live here too."""
import numpy as np

f32 = np.float32


def gaussian_radius(height, width, overlap):
    """center_utils.gaussian_radius((height, width), overlap) on fp32 arrays, term by term"""
    o = f32(overlap)
    om, op = f32(1) - o, f32(1) + o
    b1 = height + width
    c1 = width * height * om / op
    r1 = (b1 + np.sqrt(b1 * b1 - f32(4) * c1)) / f32(2)
    b2 = f32(2) * (height + width)
    c2 = om * width * height
    r2 = (b2 + np.sqrt(b2 * b2 - f32(16) * c2)) / f32(2)
    a3 = f32(4) * o
    b3 = f32(-2) * o * (height + width)
    c3 = (o - f32(1)) * width * height
    r3 = (b3 + np.sqrt(b3 * b3 - f32(4) * a3 * c3)) / f32(2)
    return np.minimum(np.minimum(r1, r2), r3)


def assign_sample(gt_boxes, gt_classes, *, num_classes, voxel_size, pc_range, out_size_factor, gaussian_overlap, min_radius, max_objs,
                  feature_map_size):
    """one sample: gt_boxes [G,9] f32, gt_classes [G] int -> dict of hm [T,C,H,W], anno_box [T,M,10], ind / mask / cat [T,M],
    gt_boxes_and_cls [M,10]; feature_map_size = (W, H)"""
    W, H = int(feature_map_size[0]), int(feature_map_size[1])
    T, C, M = len(num_classes), max(num_classes), int(max_objs)
    gt_boxes = np.asarray(gt_boxes, f32).reshape(-1, 9)
    cls = np.asarray(gt_classes).astype(np.int64).reshape(-1)
    assert len(cls) == len(gt_boxes) <= M
    hm = np.zeros((T, C, H, W), f32)
    anno = np.zeros((T, M, 10), f32)
    ind, mask, cat = np.zeros((T, M), np.int32), np.zeros((T, M), np.uint8), np.zeros((T, M), np.int32)
    gbc = np.zeros((M, 10), f32)

    keep = np.flatnonzero((cls >= 1) & (cls <= sum(num_classes)))
    keep = keep[np.argsort(cls[keep], kind="stable")]        # by task, class within the task, original index
    box, c = gt_boxes[keep], cls[keep]
    n = len(keep)
    P = f32(2 * np.pi)
    rot = box[:, 8] - np.floor(box[:, 8] / P + f32(0.5)) * P
    gbc[:n] = np.stack([box[:, 0], box[:, 1], box[:, 2], box[:, 3], box[:, 4], box[:, 5], rot, box[:, 6], box[:, 7], c.astype(f32)], 1)

    vs, pc, osf = np.asarray(voxel_size, f32), np.asarray(pc_range, f32), f32(out_size_factor)
    wc, lc = box[:, 3] / vs[0] / osf, box[:, 4] / vs[1] / osf
    ct = np.stack([(box[:, 0] - pc[0]) / vs[0] / osf, (box[:, 1] - pc[1]) / vs[1] / osf], 1)
    finite = np.isfinite(ct).all(1)
    ct_int = np.trunc(np.where(finite[:, None], ct, -1)).clip(-1, max(W, H)).astype(np.int32)
    drawn = (wc > 0) & (lc > 0) & finite & (ct_int[:, 0] >= 0) & (ct_int[:, 0] < W) & (ct_int[:, 1] >= 0) & (ct_int[:, 1] < H)
    with np.errstate(all="ignore"):
        radius = np.maximum(int(min_radius), gaussian_radius(lc, wc, gaussian_overlap).astype(np.int64))
        rows = np.concatenate([ct - ct_int.astype(f32), box[:, 2:3], np.log(box[:, 3:6]), box[:, 6:8], np.sin(rot)[:, None],
                               np.cos(rot)[:, None]], 1).astype(f32)
    base = 0
    for t, nc in enumerate(num_classes):
        member = np.flatnonzero((c > base) & (c <= base + nc))
        d = member[drawn[member]]
        slot = np.flatnonzero(drawn[member])
        anno[t, slot] = rows[d]
        ind[t, slot] = ct_int[d, 1] * W + ct_int[d, 0]
        mask[t, slot] = 1
        cat[t, slot] = c[d] - base - 1
        for i in d:
            r, (x, y) = int(radius[i]), ct_int[i]
            # gaussian2D: exp(-(x x + y y) / (2 s s)) in float64, s = (2 r + 1) / 6.  Its cut h < eps * max never fires: the smallest
            # value, at a corner of the window, is exp(-2 r r / (2 s s)) > exp(-9).
            sigma = (2 * r + 1) / 6
            left, right, top, bottom = min(x, r), min(W - x, r + 1), min(y, r), min(H - y, r + 1)
            oy, ox = np.ogrid[-top:bottom, -left:right]
            g = np.exp(-(ox * ox + oy * oy).astype(np.float64) / (2 * sigma * sigma))
            win = hm[t, c[i] - base - 1, y - top:y + bottom, x - left:x + right]
            np.maximum(win, g, out=win)
        base += nc
    return dict(hm=hm, anno_box=anno, ind=ind, mask=mask, cat=cat, gt_boxes_and_cls=gbc)


KEYS = ("hm", "anno_box", "ind", "mask", "cat", "gt_boxes_and_cls")


def assign(gt_boxes, gt_classes, **kw):
    """the batch: gt_boxes [B,G,9], gt_classes [B,G] -> the per-sample outputs stacked"""
    per = [assign_sample(b, c, **kw) for b, c in zip(gt_boxes, gt_classes)]
    return {k: np.stack([p[k] for p in per]) for k in KEYS}


# ---------------------------------------------------------------------------------------------------- accuracy conditions
def ulp_error(got, want64):
    """|got - want| in units of the fp32 spacing at want (want: float64)"""
    want64 = np.asarray(want64, np.float64)
    return np.abs(np.asarray(got, np.float64) - want64) / np.spacing(np.abs(want64).astype(f32)).astype(np.float64)


def bits_apart(a, b):
    """fp32 values a, b >= 0: how many representable values apart"""
    return np.abs(np.ascontiguousarray(a, f32).view(np.int32).astype(np.int64) - np.ascontiguousarray(b, f32).view(np.int32).astype(np.int64))


def transcendental_errors(anno_box, mask, gt_boxes_and_cls, slot_rows):
    """-> (worst log error in ulp, worst sin / cos excess over max(4 ulp, 2^-24) as a ratio <= 1 when met, worst sin / cos error in ulp)
    of the drawn rows of anno_box [B,T,M,10] against float64 of the fp32 inputs: w, l, h and the wrapped heading are read from
    gt_boxes_and_cls [B,M,10] at slot_rows [B,T,M] (the row of gt_boxes_and_cls each slot's object has)"""
    worst_log = worst_ratio = worst_trig = 0.0
    B, T = mask.shape[:2]
    for b in range(B):
        for t in range(T):
            k = np.flatnonzero(mask[b, t])
            if not len(k):
                continue
            src = gt_boxes_and_cls[b, slot_rows[b, t, k]].astype(np.float64)
            a = anno_box[b, t, k]
            worst_log = max(worst_log, float(ulp_error(a[:, 3:6], np.log(src[:, 3:6])).max()))
            want = np.stack([np.sin(src[:, 6]), np.cos(src[:, 6])], 1)
            err = np.abs(a[:, 8:10].astype(np.float64) - want)
            bound = np.maximum(4 * np.spacing(np.abs(want).astype(f32)).astype(np.float64), 2.0 ** -24)
            worst_ratio = max(worst_ratio, float((err / bound).max()))
            worst_trig = max(worst_trig, float(ulp_error(a[:, 8:10], want).max()))
    return worst_log, worst_ratio, worst_trig


def slot_rows(mask_shape, gt_classes, num_classes):
    """[B,T,M] int: the row of gt_boxes_and_cls that holds slot k of task t (rows by task, then slot); -1 for an unused slot"""
    B, T, M = mask_shape
    out = np.full((B, T, M), -1, np.int64)
    for b in range(B):
        c = np.asarray(gt_classes[b]).astype(np.int64)
        base = before = 0
        for t, nc in enumerate(num_classes):
            n = int(((c > base) & (c <= base + nc)).sum())
            out[b, t, :n] = before + np.arange(n)
            before += n
            base += nc
    return out
