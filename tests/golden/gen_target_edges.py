"""Edge-case vectors for target assignment (tests/golden/target_edges.npz), produced BY THE REFERENCE: create_target_np
(minddet/models/pointpillars/src/core/target_assigner.py:29-166) driven as TargetAssigner.assign drives it (:196-224),
similarity = rbbox2d_to_near_bbox + iou_jit(eps=0), encoding = second_box_encode, positive_fraction None -- the call of
gen_targets.py, whose target_vectors.npz this script does not touch.  Run here only:

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/gen_target_edges.py

Nothing of the reference is copied: the file holds planted / seeded inputs and what the reference returned for them.

Ground-truth ids.  create_target_np returns `positive_gt_id` = gt_ids[fg_inds] and `assigned_anchors_inds` =
inds_inside[fg_inds] (:111-115, :162-165): the ground-truth row of each anchor that a forced match or the matched
threshold labelled, and that anchor's index in the unmasked table.  fg_inds is taken BEFORE the background rule (:108,
:133), so it equals the final `labels > 0` exactly when no anchor has unmatched_thr > matched_thr; every case here keeps
unmatched_thr <= matched_thr per anchor (as every configuration of the reference does), the script asserts the equality,
and the ids are stored scattered to `<case>_gt_ids` [A] int32, -1 elsewhere.

Source of `allmasked` / `nogt_masked`: the reference too -- create_target_np accepts an empty inside set and an empty box
list (:88, :130-131) and was run on both.

Cases (all <= 600 anchors):
  planted      anchors of 2 x 4 at even integer centres, rotations 0 / 1.57, thresholds 0.6 / 0.45, plus a block of 1 x 2
               anchors with 0.5 / 0.35; boxes at integer and half-integer centres, so every IoU is a ratio of small
               integers.  Each edge is planted once at a site of its own (sites are 6 apart: their anchors are disjoint)
               and ASSERTED from the reference's own overlap matrix; the anchors are recorded as `planted_edge_<name>`
               rows (anchor, label the reference gave, gt id the reference gave) for the device tests to name.
  g1 .. g1024  seeded random boxes on a 120-anchor grid, classes 1-3, rotations in [-4, 4], a mask; the last row is a copy
               of an anchor (asserted: it is some anchor's arg-max), and g1024 carries copies of anchors at rows >= 700
               (asserted: dropping the rows from 256 / 512 on changes labels).
  a1 .. a_ragged  the first A anchors of a 612-anchor grid with 12 boxes; a_ragged = 587 = 2 * 256 + 75.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
from gen_golden import _shim  # noqa: E402

F = np.float32
BIG, SMALL = (2.0, 4.0, 2.0), (1.0, 2.0, 2.0)
ROTS = (0.0, 1.57)
FAR = [1e6, 1e6, 0.0, 1.0, 1.0, 1.0, 0.0]         # the padding row of graphs.PointPillars.train_example


def grid(nx, ny, size, x0=0.0):
    return np.array([[x0 + 2 * ix, 2 * iy, -1.0, size[0], size[1], size[2], r] for iy in range(ny) for ix in range(nx) for r in ROTS], F)


def main():
    _shim()
    from src.core import box_np_ops, target_assigner  # the reference's own modules

    def similarity(anchors, gt):
        a = box_np_ops.rbbox2d_to_near_bbox(anchors[:, [0, 1, 3, 4, 6]])
        g = box_np_ops.rbbox2d_to_near_bbox(gt[:, [0, 1, 3, 4, 6]])
        return box_np_ops.iou_jit(a, g, eps=0.0)

    def encode(boxes, anchors):
        return box_np_ops.second_box_encode(boxes, anchors)

    out = {}

    def run(name, anchors, gt, cls, mt, ut, mask):
        A = anchors.shape[0]
        anchors, gt = np.ascontiguousarray(anchors, F), np.ascontiguousarray(gt, F).reshape(-1, 7)
        cls, mt, ut = np.asarray(cls, np.int32), np.asarray(mt, F), np.asarray(ut, F)
        assert (ut <= mt).all(), name
        r = target_assigner.create_target_np(anchors, gt, similarity, encode, gt_classes=cls, matched_threshold=mt, unmatched_threshold=ut,
                                             positive_fraction=None, rpn_batch_size=512, norm_by_num_examples=False, box_code_size=7,
                                             anchors_mask=mask.astype(bool))
        labels = r["labels"].astype(np.int32)
        ids = np.full((A,), -1, np.int32)
        ids[r["assigned_anchors_inds"]] = r["positive_gt_id"]
        assert ((ids >= 0) == (labels > 0)).all(), name + ": fg_inds differs from labels > 0"
        for k, v in dict(anchors=anchors, gt=gt, cls=cls, mt=mt, ut=ut, mask=mask.astype(np.uint8), labels=labels,
                         targets=r["bbox_targets"].astype(F), weights=r["bbox_outside_weights"].astype(F), gt_ids=ids).items():
            out[name + "_" + k] = v
        print(name, "anchors", A, "gt", gt.shape[0], "inside", int(mask.sum()), "pos", int((labels > 0).sum()), "neg", int((labels == 0).sum()))
        return labels, ids

    # ------------------------------------------------------------------------------------------------ planted
    NX, NY = 18, 9
    anchors = np.concatenate([grid(NX, NY, BIG), grid(4, 3, SMALL, x0=100.0)])
    nbig = NX * NY * 2
    A = anchors.shape[0]

    def ai(x, y, r):                                 # big anchor at centre (x, y), r = 0 / 1 for rotation 0 / 1.57
        return ((y // 2) * NX + x // 2) * 2 + r

    def si(x, y, r):                                 # small anchor
        return nbig + ((y // 2) * 4 + (x - 100) // 2) * 2 + r

    gt, cls = [], []

    def box(x, y, w=2.0, l=4.0, rot=0.0, c=1, z=-1.0, h=2.0):
        gt.append([x, y, z, w, l, h, rot]); cls.append(c)
        return len(gt) - 1

    p4 = F(np.pi / 4)
    inf = F(np.inf)
    b_on = box(2, 2, c=1)                            # site (2, 2): a box on an anchor ...
    b_in = box(2, 3.5, 1.0, 1.0, c=2, z=-0.5, h=1.0)  # ... and a 1 x 1 box inside that anchor: it forces the anchor, whose arg-max stays b_on
    b_far_mid = box(*FAR[:2], FAR[3], FAR[4], FAR[6], 2, FAR[2], FAR[5])
    b_thr = box(8, 2, c=3)                           # site (8, 2): threshold equalities on the neighbours of a box on an anchor
    b_t1 = box(13, 2, c=1)                           # site (14, 2): anchor (14, 2) midway between two boxes, bit-equal IoU 1/3
    b_t2 = box(15, 2, c=2)
    b_mid = box(21, 2, c=3, h=1.5)                   # site (20, 2): one box midway between two anchors: four tied column maxima
    b_small = box(26, 2, 1.0, 1.0, c=2)              # site (26, 2): forced at IoU 1/8, below unmatched_thr
    b_mask = box(32, 2, c=1)                         # site (32, 2): a box on an anchor that the mask removes
    b_dup = box(2, 8.5, c=1)                         # site (2, 8): duplicated further down with class 3
    rot_vals = [p4, np.nextafter(p4, inf), np.nextafter(p4, F(0)), -p4, np.nextafter(-p4, -inf), np.nextafter(-p4, F(0)),
                F(3 * np.pi / 4), F(4.0), F(-3.5), F(100.0), F(np.pi), F(-3 * np.pi / 4)]
    rot_sites = [(8, 8), (14, 8), (20, 8), (26, 8), (32, 8), (2, 14), (8, 14), (14, 14), (20, 14), (26, 14), (32, 14), (102, 2)]
    b_rot = [box(x, y, *(SMALL[:2] if x >= 100 else BIG[:2]), rot=r, c=1 + i % 3) for i, ((x, y), r) in enumerate(zip(rot_sites, rot_vals))]
    b_s4 = box(106, 3, 1.0, 4.0, c=3)                # small block: covers two 1 x 2 anchors, IoU 1/2 = their matched_thr
    b_dup2 = box(2, 8.5, c=3)
    b_far_end = box(*FAR[:2], FAR[3], FAR[4], FAR[6], 1, FAR[2], FAR[5])
    gt, cls = np.array(gt, F), np.array(cls, np.int32)
    G = gt.shape[0]

    mt = np.concatenate([np.full(nbig, 0.6, F), np.full(A - nbig, 0.5, F)])
    ut = np.concatenate([np.full(nbig, 0.45, F), np.full(A - nbig, 0.35, F)])
    mask = np.ones((A,), bool)
    mask[ai(32, 2, 0)] = False                       # the overall best anchor of b_mask
    mask[[ai(0, 16, 0), ai(34, 16, 1), si(100, 4, 1)]] = False   # three anchors no box touches

    ov = similarity(anchors, gt)                     # the reference's own overlap matrix, all anchors
    assert ov.dtype == np.float32
    a_mt, a_mt_up = ai(8, 0, 0), ai(8, 4, 0)         # IoU 1/3 with b_thr, by symmetry bit-equal
    a_ut, a_ut_up = ai(8, 0, 1), ai(8, 4, 1)         # IoU 1/7
    assert ov[a_mt, b_thr] == ov[a_mt_up, b_thr] and ov[a_ut, b_thr] == ov[a_ut_up, b_thr], "threshold twins are not bit-equal"
    mt[a_mt], mt[a_mt_up] = ov[a_mt, b_thr], np.nextafter(ov[a_mt_up, b_thr], inf)
    ut[[a_mt, a_mt_up]] = 0.25
    ut[a_ut], ut[a_ut_up] = ov[a_ut, b_thr], np.nextafter(ov[a_ut_up, b_thr], inf)

    labels, ids = run("planted", anchors, gt, cls, mt, ut, mask)

    ovm = ov[mask]                                   # what the assigner sees
    col = ovm.max(0)
    inside = np.where(mask)[0]
    amax, arg = ov.max(1), ov.argmax(1)
    is_colmax = (ov == col[None, :]) & (col[None, :] > 0) & mask[:, None]
    edges = {}

    def edge(name, rows):
        rows = [(a, int(labels[a]), int(ids[a])) for a in rows]
        edges[name] = np.array(rows, np.int32).reshape(-1, 3)

    a = ai(2, 2, 0)
    assert is_colmax[a, b_in] and arg[a] == b_on and cls[b_in] != cls[b_on], "forced match with a different arg-max is not planted"
    assert labels[a] == cls[b_on] and ids[a] == b_on, "forced match with a different arg-max: the reference did not take the arg-max"
    edge("forced_other_argmax", [a])
    a = ai(2, 4, 0)                                  # forced by b_in at 1/8, arg-max b_on at 1/3: both below unmatched_thr
    assert is_colmax[a, b_in] and arg[a] == b_on and amax[a] < ut[a] and labels[a] == cls[b_on] and ids[a] == b_on, \
        "forced match below unmatched_thr with a different arg-max is not planted"
    edge("forced_other_argmax_below_ut", [a])
    rows = [ai(26, 2, 0), ai(26, 2, 1)]
    for a in rows:
        assert is_colmax[a, b_small] and amax[a] == F(0.125) and amax[a] < ut[a] and labels[a] == cls[b_small] and ids[a] == b_small, \
            "forced match under the background rule is not planted"
    edge("forced_below_ut", rows)
    rows = [ai(20, 2, 0), ai(20, 2, 1), ai(22, 2, 0), ai(22, 2, 1)]
    assert len({ov[a, b_mid].tobytes() for a in rows}) == 1 and all(is_colmax[a, b_mid] and ids[a] == b_mid for a in rows) and \
        is_colmax[:, b_mid].sum() == 4, "anchors tied for one box's column maximum are not planted"
    edge("tied_anchors", rows)
    rows = [ai(14, 2, 0), ai(14, 2, 1)]
    for a in rows:
        assert ov[a, b_t1] == ov[a, b_t2] == amax[a] and b_t1 < b_t2 and cls[b_t1] != cls[b_t2] and ids[a] == b_t1, \
            "an anchor tied between two boxes is not planted"
    assert ((((ov == amax[:, None]) & (ov > 0)).sum(1) >= 2) & mask).sum() >= 3, "fewer than three anchors with tied row maxima"
    edge("tied_boxes", rows)
    a = ai(2, 8, 0)
    assert (gt[b_dup] == gt[b_dup2]).all() and cls[b_dup] != cls[b_dup2] and arg[a] == b_dup and amax[a] >= mt[a] and ids[a] == b_dup \
        and labels[a] == cls[b_dup], "a duplicated ground-truth row with another class is not planted"
    edge("duplicate_row", [a])
    a = ai(2, 2, 0)
    assert ov[a, b_on] == 1 and (gt[b_on] == anchors[a]).all(), "a box on an anchor is not planted"
    edge("on_anchor", [a, ai(8, 2, 0)])
    assert ov[a_mt, b_thr] == mt[a_mt] == amax[a_mt] and not is_colmax[a_mt].any() and labels[a_mt] == cls[b_thr], \
        "amax == matched_thr is not planted as foreground"
    assert amax[a_mt_up] < mt[a_mt_up] and amax[a_mt_up] >= ut[a_mt_up] and not is_colmax[a_mt_up].any() and labels[a_mt_up] == -1, \
        "amax one ulp below matched_thr is not planted as ignore"
    edge("mt_equal", [a_mt]); edge("mt_above", [a_mt_up])
    assert amax[a_ut] == ut[a_ut] and not is_colmax[a_ut].any() and labels[a_ut] == -1, "amax == unmatched_thr is not planted as ignore"
    assert amax[a_ut_up] < ut[a_ut_up] and not is_colmax[a_ut_up].any() and labels[a_ut_up] == 0, "amax one ulp below unmatched_thr is not background"
    edge("ut_equal", [a_ut]); edge("ut_above", [a_ut_up])
    a = ai(32, 2, 0)
    rows = [r for r in np.where(is_colmax[:, b_mask])[0]]
    assert ov[:, b_mask].argmax() == a and not mask[a] and ov[a, b_mask] > col[b_mask] > 0 and len(rows) >= 1 and \
        all(amax[r] < ut[r] and ids[r] == b_mask for r in rows), "the masked-out best anchor of a box is not planted"
    edge("masked_best", [a]); edge("masked_best_forced", rows)
    for b in (b_far_mid, b_far_end):
        assert (ov[:, b] == 0).all() and not (ids == b).any(), "a box nothing overlaps is not planted"
    assert 0 < b_far_mid < G - 1 and b_far_end == G - 1 and (labels[(amax == 0) & mask] == 0).all() and ((amax == 0) & mask).sum() > 50, \
        "the far boxes are not between real boxes and at the end, or an anchor nothing overlaps is not background"
    rows = []
    for b, (x, y), r in zip(b_rot, rot_sites, rot_vals):
        pair = [si(x, y, 0), si(x, y, 1)] if x >= 100 else [ai(x, y, 0), ai(x, y, 1)]
        on = [q for q in pair if ov[q, b] == 1]
        assert len(on) == 1 and ids[on[0]] == b, "rotation-boundary box %d (rot %r) is not on exactly one anchor" % (b, r)
        rows += pair
    swapped = [int(ov[ai(x, y, 1) if x < 100 else si(x, y, 1), b] == 1) for b, (x, y) in zip(b_rot, rot_sites)]
    assert swapped[0] == 0 and swapped[1] == 1 and swapped[2] == 0 and swapped[3] == 0 and swapped[4] == 1 and swapped[5] == 0, \
        "the near-box swap does not flip one ulp above +-pi/4: %r" % (swapped,)
    assert 0 < sum(swapped[6:]) < len(swapped[6:]), "rotations beyond the first period swap all or none"
    edge("rotation", rows)
    out["planted_rot_boxes"] = np.array(b_rot, np.int32)
    out["planted_far_boxes"] = np.array([b_far_mid, b_far_end], np.int32)
    rows = [si(106, 2, 0), si(106, 4, 0)]
    for a in rows:
        assert amax[a] == mt[a] == F(0.5) and ids[a] == b_s4, "the second size class is not matched at its own threshold"
    edge("small_class", rows)
    outside = np.where(~mask)[0]
    assert (labels[outside] == -1).all() and (ids[outside] == -1).all(), "a masked-out anchor has a label or an id"
    for k, v in edges.items():
        out["planted_edge_" + k] = v
    print("planted edges:", {k: v[:, 0].tolist() for k, v in edges.items()}, "swapped", swapped)

    # ------------------------------------------------------------------------------------------------ seeded cases
    rng = np.random.default_rng(41)

    def thresholds(anc):
        r1 = anc[:, 6] != 0
        return np.where(r1, 0.5, 0.6).astype(F), np.where(r1, 0.35, 0.45).astype(F)

    def boxes(n, xmax, ymax):
        g = np.zeros((n, 7), F)
        g[:, 0] = np.round(rng.uniform(-1, xmax + 1, n) * 2) / 2
        g[:, 1] = np.round(rng.uniform(-1, ymax + 1, n) * 2) / 2
        g[:, 2] = rng.uniform(-2, 0, n)              # z and the height do not enter the IoU: arbitrary values for the encoding
        g[:, 3] = rng.choice([1.0, 1.5, 2.0, 3.0], n)
        g[:, 4] = rng.choice([2.0, 3.0, 4.0, 5.0], n)
        g[:, 5] = rng.uniform(1.0, 2.5, n)
        g[:, 6] = rng.uniform(-4, 4, n)
        return g, rng.integers(1, 4, n).astype(np.int32)

    small = grid(10, 6, BIG)                         # 120 anchors
    for n in (1, 255, 256, 257, 1024):
        g, c = boxes(n, 18, 10)
        m = rng.uniform(0, 1, small.shape[0]) < 0.8
        if n == 1:
            g[0, :2] = [6.0, 4.5]
        free = np.where(m)[0]
        if n == 1024:                                # the boxes that decide most labels sit at rows >= 700
            sel = rng.choice(free, 40, replace=False)
            g[700:740] = small[sel]
            c[700:740] = 1 + np.arange(40) % 3
            free = np.setdiff1d(free, sel)
        if n > 1:                                    # the last row is a copy of an anchor: a table one row short changes an id
            g[n - 1] = small[rng.choice(free)]
        mt_, ut_ = thresholds(small)
        lab, gid = run("g%d" % n, small, g, c, mt_, ut_, m)
        if n > 1:
            assert (gid == n - 1).any(), "g%d: the last row is nobody's arg-max" % n
        if n == 1024:
            for cut in (256, 512):
                r = target_assigner.create_target_np(small, g[:cut], similarity, encode, gt_classes=c[:cut], matched_threshold=mt_,
                                                     unmatched_threshold=ut_, positive_fraction=None, rpn_batch_size=512,
                                                     norm_by_num_examples=False, box_code_size=7, anchors_mask=m)
                assert (r["labels"] != lab).sum() >= 10, "g1024: the first %d rows decide the labels" % cut
    wide = grid(18, 17, BIG)                         # 612 anchors
    for name, n in (("a1", 1), ("a255", 255), ("a256", 256), ("a257", 257), ("a_ragged", 587)):
        anc = wide[:n]
        g, c = boxes(12, float(anc[:, 0].max()), float(anc[:, 1].max()))
        if n == 1:
            g[0] = anc[0]; g[0, 1] = 0.5
        m = rng.uniform(0, 1, n) < 0.8 if n > 1 else np.ones((1,), bool)
        lab, _ = run(name, anc, g, c, *thresholds(anc), m)
        assert (lab > 0).any(), name
    g, c = boxes(12, 18, 10)
    run("allmasked", small, g, c, *thresholds(small), np.zeros((small.shape[0],), bool))
    m = rng.uniform(0, 1, small.shape[0]) < 0.5
    run("nogt_masked", small, np.zeros((0, 7), F), np.zeros((0,), np.int32), *thresholds(small), m)
    out["case_names"] = np.array(["planted", "g1", "g255", "g256", "g257", "g1024", "a1", "a255", "a256", "a257", "a_ragged", "allmasked",
                                  "nogt_masked"])
    np.savez_compressed(os.path.join(HERE, "target_edges.npz"), **out)


if __name__ == "__main__":
    main()
