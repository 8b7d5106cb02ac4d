"""What md_assign_targets (csrc/targets.hip) has to compute, in plain code, and the mistakes it must not make.

`cases()` loads tests/golden/target_edges.npz: planted and seeded inputs with the outputs of the reference's own
create_target_np (tests/golden/gen_target_edges.py).  `judge()` is a per-anchor loop written from the operator's contract, not
from oracle/np_ops.py::create_target (which it never calls): the near box and the IoU in the reference's float32 operation
order, the FIRST arg-max, column maxima over the masked-in anchors, forced matches that survive the background rule, the
encoding's linear terms in float32 and its three logarithms in float64 of the float32 quotient.  With `variant` it makes
exactly one deliberate mistake; tests/test_targets_cpu.py demands that the fixture catches every one of them, so an edge that
stops being planted fails there and not silently on the device.

Contract limits: unmatched_thr <= matched_thr for every anchor (the reference then labels by fg-before-background order,
which no configuration uses and the operator does not reproduce); no NaN and no negative sizes."""
import os

import numpy as np

F = np.float32
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "target_edges.npz")
FIELDS = ("anchors", "gt", "cls", "mt", "ut", "mask")
VARIANTS = {
    "last_argmax": "last arg-max instead of first",
    "forced_takes_forcing_box": "forced anchors use the forcing box instead of their arg-max",
    "forced_loses_to_background": "forced anchors lose to the background rule",
    "matched_gt": "> for matched_thr",
    "unmatched_le": "<= for unmatched_thr",
    "colmax_ignores_mask": "column maxima over all anchors instead of the masked-in ones",
    "empty_box_forces": "an unoverlapped box forces every anchor with IoU 0",
    "table_256": "the box table truncated to its first 256 rows",
    "swap_ge": "the near-box swap with >=",
}
EDGE_MESSAGES = {
    "forced_other_argmax": "forced match took the forcing box, not the anchor's own arg-max",
    "forced_other_argmax_below_ut": "forced match below unmatched_thr with another arg-max: relabelled or wrong box",
    "forced_below_ut": "forced match lost to the background rule",
    "tied_anchors": "anchors with bit-equal IoU to one box were not all forced",
    "tied_boxes": "an anchor tied between two boxes did not take the first",
    "duplicate_row": "a duplicated ground-truth row: the later copy won",
    "on_anchor": "a box on an anchor was not matched to it",
    "mt_equal": "amax == matched_thr is foreground (>=)",
    "mt_above": "amax one ulp below matched_thr is not foreground",
    "ut_equal": "amax == unmatched_thr is ignore, not background (<)",
    "ut_above": "amax one ulp below unmatched_thr is background",
    "masked_best": "a masked-out anchor got something else than label -1 / id -1",
    "masked_best_forced": "the best masked-in anchor was not forced when the overall best is masked out",
    "rotation": "the near-box swap is wrong at a rotation boundary",
    "small_class": "the second size class was not judged by its own thresholds",
}
_cache = {}


def fixture():
    if "z" not in _cache:
        with np.load(FIXTURE) as z:
            _cache["z"] = {k: z[k] for k in z.files}
    return _cache["z"]


def case_names():
    return [str(n) for n in fixture()["case_names"]]


def cases():
    """{name: dict(anchors, gt, cls, mt, ut, mask, labels, targets, weights, gt_ids)}; read-only arrays"""
    if "cases" not in _cache:
        z, out = fixture(), {}
        for n in case_names():
            out[n] = {k: z[n + "_" + k] for k in FIELDS + ("labels", "targets", "weights", "gt_ids")}
            for v in out[n].values():
                v.setflags(write=False)
        _cache["cases"] = out
    return _cache["cases"]


def edges():
    """{name: int32 [n, 3] rows (anchor, label, gt id) of the `planted` case}"""
    z = fixture()
    return {k[len("planted_edge_"):]: z[k] for k in z if k.startswith("planted_edge_")}


def _near(b, ge=False):
    """[n,7] -> (x0, y0, x1, y1) float32 columns: the axis-aligned box nearest to the rotated one"""
    pi = F(np.pi)
    r = b[:, 6]
    lp = np.abs(r - np.floor(r / pi + F(0.5)) * pi)
    swap = lp >= F(np.pi / 4) if ge else lp > F(np.pi / 4)
    dx, dy = np.where(swap, b[:, 4], b[:, 3]), np.where(swap, b[:, 3], b[:, 4])
    two = F(2)
    return b[:, 0] - dx / two, b[:, 1] - dy / two, b[:, 0] + dx / two, b[:, 1] + dy / two


def _iou_row(ab, gb):
    """one anchor's near box against every ground-truth near box, float32, eps = 0"""
    gx0, gy0, gx1, gy1 = gb
    qa = (gx1 - gx0) * (gy1 - gy0)
    iw = np.minimum(ab[2], gx1) - np.maximum(ab[0], gx0)
    ih = np.minimum(ab[3], gy1) - np.maximum(ab[1], gy0)
    ua = (ab[2] - ab[0]) * (ab[3] - ab[1]) + qa - iw * ih
    ok = (iw > 0) & (ih > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = iw * ih / ua
    return np.where(ok, v, F(0)).astype(F)


def judge(anchors, gt, cls, mt, ut, mask, variant=None):
    """-> labels [A] i32, targets [A,7] float64 (columns 0, 1, 2, 6 hold float32 values; 3, 4, 5 = log in float64 of the float32
    quotient), weights [A] f32, gt_ids [A] i32"""
    assert variant is None or variant in VARIANTS, variant
    anchors, gt = np.asarray(anchors, F).reshape(-1, 7), np.asarray(gt, F).reshape(-1, 7)
    A, G = anchors.shape[0], gt.shape[0]
    if variant == "table_256":
        G = min(G, 256)
        gt = gt[:G]
    inside = np.ones((A,), bool) if mask is None or len(mask) == 0 else np.asarray(mask).astype(bool)
    labels, gt_ids = np.full((A,), -1, np.int32), np.full((A,), -1, np.int32)
    targets, weights = np.zeros((A, 7), np.float64), np.zeros((A,), F)
    if G == 0:
        labels[inside] = 0
        return labels, targets, weights, gt_ids
    ge = variant == "swap_ge"
    an, gb = np.stack(_near(anchors, ge), 1), _near(gt, ge)
    rows = [_iou_row(an[a], gb) for a in range(A)]
    colmax = np.zeros((G,), F)
    for a in range(A):
        if inside[a] or variant == "colmax_ignores_mask":
            colmax = np.maximum(colmax, rows[a])
    for a in range(A):
        if not inside[a]:
            continue
        v = rows[a]
        amax = v.max()
        hits = np.flatnonzero(v == amax)
        arg = int(hits[-1] if variant == "last_argmax" else hits[0])
        forcing = np.flatnonzero((v == colmax) & ((colmax > 0) | (variant == "empty_box_forces")))
        forced = forcing.size > 0
        if forced and variant == "forced_takes_forcing_box":
            arg = int(forcing[0])
        matched = amax > mt[a] if variant == "matched_gt" else amax >= mt[a]
        unmatched = amax <= ut[a] if variant == "unmatched_le" else amax < ut[a]
        if variant == "forced_loses_to_background" and unmatched and not matched:
            forced = False
        if forced or matched:
            labels[a] = cls[arg]
        elif unmatched:
            labels[a] = 0
        if labels[a] > 0:
            g, n = gt[arg], anchors[a]
            two = F(2)
            diagonal = np.sqrt(n[4] * n[4] + n[3] * n[3])
            targets[a] = [(g[0] - n[0]) / diagonal, (g[1] - n[1]) / diagonal, ((g[2] + g[5] / two) - (n[2] + n[5] / two)) / n[5],
                          np.log(np.float64(g[3] / n[3])), np.log(np.float64(g[4] / n[4])), np.log(np.float64(g[5] / n[5])), g[6] - n[6]]
            weights[a] = 1
            gt_ids[a] = arg
    return labels, targets, weights, gt_ids


def log_ulps(got, want64):
    """fp32 bit distance of got [.., 3] float32 to want64 rounded to float32, and the absolute error against want64"""
    got = np.ascontiguousarray(got, F)
    want = np.ascontiguousarray(want64.astype(F))
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)), np.abs(got.astype(np.float64) - want64)
