"""The contract of the COCO bbox AP operators (include/minddet_hip_cocoeval.h), restated in numpy per cell, and the test set both
tests/test_coco_eval_device_cpu.py and tests/test_coco_eval_device_gpu.py use.  The judge of the operators is the host evaluator
(minddet_amd/coco_eval.py); this file is the judge of the restatement: its tables must equal COCOBboxEval's bit for bit, and each of
the six planted defects (DEFECTS) must change them on the set below -- if one does not, the set is too weak.

  to_float_recipe   the header's to_float, the exact product error taken from fractions
  rows_image        md_coco_eval_rows for one image
  match_cell        md_coco_eval_match for one (cell, area range), all thresholds
  accumulate        md_coco_eval_accumulate
  tables            the three on a pack (numpy views of coco_eval.pack_coco(device="cpu"))
  test_set          16 generated images x 3 categories + the hand-made cells
"""
import functools
from fractions import Fraction

import numpy as np

DEFECTS = ("lowest_row", "crowd_once", "ignored_beats", "gt_bar", "exclusive_area", "unstable_order")
MAX_CELL_DETS = 100
EPS = 2.0 ** -52


def to_float_recipe(v):
    """float("{:.2f}".format(v)) without formatting: p = v 100 rounded, e its exact error, ties of p decided by the sign of e"""
    v = float(v)
    if v != v or v in (float("inf"), float("-inf")):
        return v
    p = v * 100.0
    e = Fraction(v) * 100 - Fraction(p)
    n = float(np.rint(p))
    f = p - n
    if f == 0.5 and e > 0:
        n += 1.0
    if f == -0.5 and e < 0:
        n -= 1.0
    return n / 100.0


def rows_image(dets, count, label_to_k, Kc):
    """dets [max_det,6] f32, count -> dict of the image's block: box [max_det,4], area, score, cat, rank, src and beg / cnt [Kc] (beg
    relative to the block)"""
    max_det = len(dets)
    n = min(max(int(count), 0), max_det)
    d = np.asarray(dets, np.float32).astype(np.float64)
    taken = []
    for r in range(n):
        lab = d[r, 5]
        if not (lab > -1.0 and lab < len(label_to_k)):
            continue
        k = int(label_to_k[int(lab)])
        if 0 <= k < Kc:
            taken.append((k, -to_float_recipe(d[r, 4]), r))
    out = dict(box=np.zeros((max_det, 4)), area=np.zeros(max_det), score=np.zeros(max_det), cat=np.full(max_det, Kc, np.int32),
               rank=np.zeros(max_det, np.int32), src=np.full(max_det, -1, np.int32), beg=np.zeros(Kc, np.int32), cnt=np.zeros(Kc, np.int32))
    at = 0
    for k in range(Kc):
        cell = sorted(t for t in taken if t[0] == k)[:MAX_CELL_DETS]
        out["beg"][k], out["cnt"][k] = at, len(cell)
        for rank, (_, neg, r) in enumerate(cell):
            w, h = to_float_recipe(d[r, 2] - d[r, 0]), to_float_recipe(d[r, 3] - d[r, 1])
            out["box"][at] = [to_float_recipe(d[r, 0]), to_float_recipe(d[r, 1]), w, h]
            out["area"][at], out["score"][at], out["cat"][at], out["rank"][at], out["src"][at] = w * h, -neg, k, rank, r
            at += 1
    return out


def iou_pair(d, g, crowd):
    iw = max(min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0]), 0.0)
    ih = max(min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1]), 0.0)
    inter = iw * ih
    da, ga = d[2] * d[3], g[2] * g[3]
    union = da if crowd else (da + ga) - inter
    return inter / union if union > 0 else 0.0


def match_cell(gt_box, gt_area, gt_crowd, gt_ignore, dt_box, dt_area, iou_thr, lo, hi, defect=None):
    """-> dtm [T,D] (the cell's ground-truth index or -1), dt_ig [T,D] bool, the counted ground truths"""
    G, D, T = len(gt_box), len(dt_box), len(iou_thr)
    if defect == "exclusive_area":
        ign = [bool(gt_ignore[g]) or gt_area[g] <= lo or gt_area[g] >= hi for g in range(G)]
    else:
        ign = [bool(gt_ignore[g]) or gt_area[g] < lo or gt_area[g] > hi for g in range(G)]
    iou = np.array([[iou_pair(dt_box[d], gt_box[g], gt_crowd[g]) for g in range(G)] for d in range(D)]).reshape(D, G)
    dtm, dt_ig = -np.ones((T, D), np.int32), np.zeros((T, D), bool)
    for t in range(T):
        bar = min(iou_thr[t], 1 - 1e-10)
        held = [False] * G
        for d in range(D):
            best = None                                        # (counted, iou, row)
            for g in range(G):
                if held[g] and not (gt_crowd[g] and defect != "crowd_once"):
                    continue
                if not (iou[d, g] > bar if defect == "gt_bar" else iou[d, g] >= bar):
                    continue
                key = (0 if defect == "ignored_beats" else int(not ign[g]), iou[d, g], -g if defect == "lowest_row" else g)
                if best is None or key > best[0]:
                    best = (key, g)
            if best is None:
                dt_ig[t, d] = dt_area[d] < lo or dt_area[d] > hi
            else:
                g = best[1]
                held[g] = True
                dtm[t, d], dt_ig[t, d] = g, ign[g]
    return dtm, dt_ig, sum(not i for i in ign)


def accumulate(dt_score, dt_cat, dt_rank, dtm, dt_ig, cell_ngt, Kc, rec_thr, max_dets, defect=None):
    """dtm, dt_ig [A,T,Dt], cell_ngt [A, I Kc] -> precision [T,R,Kc,A,M], recall [T,Kc,A,M], n_gt [A,Kc]"""
    A, T, Dt = dtm.shape
    R, M = len(rec_thr), len(max_dets)
    rows = np.arange(Dt)
    tie = -rows if defect == "unstable_order" else rows
    order = np.array(sorted(range(Dt), key=lambda r: (dt_cat[r], -dt_score[r], tie[r])), np.int64)
    n_gt = cell_ngt.reshape(A, -1, Kc).sum(1)
    precision, recall = -np.ones((T, R, Kc, A, M)), -np.ones((T, Kc, A, M))
    for k in range(Kc):
        lst = order[dt_cat[order] == k]
        for a in range(A):
            if n_gt[a, k] == 0:
                continue
            for m in range(M):
                sub = lst[dt_rank[lst] < max_dets[m]]
                for t in range(T):
                    mt, ig = dtm[a, t, sub] >= 0, dt_ig[a, t, sub] != 0
                    tp, fp = np.cumsum(mt & ~ig).astype(float), np.cumsum(~mt & ~ig).astype(float)
                    rc = tp / n_gt[a, k]
                    pr = tp / (fp + tp + EPS)
                    env = np.maximum.accumulate(pr[::-1])[::-1]        # the maximum to the right
                    first = np.searchsorted(rc, rec_thr, side="left")
                    q = np.zeros(R)
                    q[first < len(sub)] = env[first[first < len(sub)]]
                    precision[t, :, k, a, m] = q
                    recall[t, k, a, m] = rc[-1] if len(sub) else 0.0
    return precision, recall, n_gt.astype(np.int32)


def pack_numpy(p):
    """the tensors of a PackedCoco as numpy arrays"""
    names = ("gt_beg", "gt_cnt", "dt_beg", "dt_cnt", "gt_box", "gt_area", "gt_crowd", "gt_ignore", "dt_box", "dt_area", "dt_score", "dt_cat", "dt_rank")
    return {n: getattr(p, n).cpu().numpy() for n in names}


def tables(z, Kc, iou_thr, rec_thr, area_rng, max_dets, defect=None):
    """the contract on the arrays of pack_numpy -> dict(dtm [A,T,Dt] packed rows, dt_ig, cell_ngt, precision, recall, n_gt)"""
    A, T, Dt, C = len(area_rng), len(iou_thr), len(z["dt_area"]), len(z["gt_beg"])
    dtm, dt_ig, cell_ngt = -np.ones((A, T, Dt), np.int32), np.zeros((A, T, Dt), np.uint8), np.zeros((A, C), np.int32)
    for c in range(C):
        g0, gn, d0, dn = int(z["gt_beg"][c]), int(z["gt_cnt"][c]), int(z["dt_beg"][c]), int(z["dt_cnt"][c])
        gs, ds = slice(g0, g0 + gn), slice(d0, d0 + dn)
        for a, (lo, hi) in enumerate(area_rng):
            m, ig, n = match_cell(z["gt_box"][gs], z["gt_area"][gs], z["gt_crowd"][gs], z["gt_ignore"][gs], z["dt_box"][ds], z["dt_area"][ds], iou_thr,
                                  lo, hi, defect)
            dtm[a, :, ds], dt_ig[a, :, ds], cell_ngt[a, c] = np.where(m >= 0, m + g0, -1), ig, n
    precision, recall, n_gt = accumulate(z["dt_score"], z["dt_cat"], z["dt_rank"], dtm, dt_ig, cell_ngt, Kc, rec_thr, max_dets, defect)
    return dict(dtm=dtm, dt_ig=dt_ig, cell_ngt=cell_ngt, precision=precision, recall=recall, n_gt=n_gt)


# ----------------------------------------------------------------------------- the test set
CATS = (1, 2, 3)
SIZES = ((32, 32), (96, 96), (16, 16), (48, 40), (64, 64), (32, 64))     # areas of exactly 1024 and 9216 among them


def _gt(img, cat, box, crowd=0, **kw):
    return dict(image_id=img, category_id=cat, bbox=[float(v) for v in box], iscrowd=int(crowd), **kw)


def _dt(img, cat, box, score):
    return dict(image_id=img, category_id=cat, bbox=[float(v) for v in box], score=float(score))


def generated(seed=7, images=16):
    """boxes on an 8-pixel grid (equal IoUs), duplicated ground truths, 15 % crowds, scores in steps of 0.05 (ties inside cells and across
    images); the detection records are shuffled, so record order is not image order"""
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for img in range(1, images + 1):
        for cat in CATS:
            for _ in range(int(rng.integers(0, 5))):
                x, y = (8 * rng.integers(0, 24, 2)).tolist()
                w, h = SIZES[int(rng.integers(0, len(SIZES)))]
                g = _gt(img, cat, (x, y, w, h), crowd=rng.random() < 0.15)
                if rng.random() < 0.1:
                    g["ignore"] = 1
                gts.append(g)
                if rng.random() < 0.25:
                    gts.append(dict(g))                            # a duplicate: two ground truths at one IoU
                for _ in range(int(rng.integers(1, 3))):           # detections around it, on the grid
                    dx, dy = (8 * rng.choice([-1, 0, 0, 0, 1], 2)).tolist()
                    dw, dh = (w, h) if rng.random() < 0.8 else SIZES[int(rng.integers(0, len(SIZES)))]
                    dts.append(_dt(img, cat, (x + dx, y + dy, dw, dh), round(0.05 * int(rng.integers(1, 20)), 2)))
            for _ in range(int(rng.integers(0, 2))):               # and some anywhere
                x, y = (8 * rng.integers(0, 24, 2)).tolist()
                w, h = SIZES[int(rng.integers(0, len(SIZES)))]
                dts.append(_dt(img, cat, (x, y, w, h), round(0.05 * int(rng.integers(1, 12)), 2)))
    return gts, [dts[i] for i in rng.permutation(len(dts))]


def hand_made(first_img=101):
    """one image per cell: -> (ground truths, detections, {name: (image id, category id)})"""
    rng = np.random.default_rng(11)
    gts, dts, where = [], [], {}
    img = first_img

    def cell(name, cat=1):
        nonlocal img
        where[name] = (img, cat)
        img += 1
        return img - 1

    i = cell("dets_only")
    dts += [_dt(i, 1, (0, 0, 32, 32), 0.9), _dt(i, 1, (8, 8, 200, 200), 0.4)]
    i = cell("gts_only", 5)                                        # category 5 has ground truths and no detection anywhere
    gts += [_gt(i, 5, (0, 0, 32, 32)), _gt(i, 5, (40, 0, 96, 96))]
    for n in (65, 130, 256):                                       # chunk edges and the limit: a 16-wide lattice of overlapping boxes
        i = cell(f"gts_{n}", 3)
        for j in range(n):
            gts.append(_gt(i, 3, (8 * (j % 16), 8 * (j // 16), 16, 16), crowd=(j % 11 == 5)))
        for j in rng.permutation(n)[:24].tolist():                 # detections on and next to ground truths of every chunk
            dts.append(_dt(i, 3, (8 * (j % 16), 8 * (j // 16) + (8 if j % 3 == 0 else 0), 16, 16), round(0.05 * (1 + j % 19), 2)))
        dts.append(_dt(i, 3, (8 * ((n - 1) % 16), 8 * ((n - 1) // 16), 16, 16), 0.95))      # the last ground truth's own
    i = cell("dets_140")
    gts += [_gt(i, 1, (0, 0, 32, 32)), _gt(i, 1, (64, 64, 32, 32))]
    for j in range(140):                                           # the cut at 100: the best of the last ones would match
        dts.append(_dt(i, 1, (64, 64, 32, 32) if j == 139 else (8 * (j % 5), 8 * (j % 3), 32, 32), 0.99 if j == 139 else round(0.05 + 0.005 * (j % 100), 3)))
    i = cell("all_crowd", 2)
    gts += [_gt(i, 2, (0, 0, 64, 64), crowd=1), _gt(i, 2, (32, 32, 64, 64), crowd=1)]
    dts += [_dt(i, 2, (0, 0, 32, 32), 0.8), _dt(i, 2, (8, 8, 32, 32), 0.7), _dt(i, 2, (40, 40, 32, 32), 0.6), _dt(i, 2, (200, 200, 16, 16), 0.5)]
    i = cell("crowd_and_counted", 3)                               # a crowd with the larger IoU must not beat the counted ground truth
    gts += [_gt(i, 3, (0, 0, 16, 16)), _gt(i, 3, (0, 0, 16, 12), crowd=1)]
    dts += [_dt(i, 3, (0, 0, 16, 12), 0.9)]
    i = cell("iou_half")                                           # 128 / 256 and 192 / 256: exactly 0.5 and 0.75, which meet their thresholds
    gts += [_gt(i, 1, (0, 0, 16, 16)), _gt(i, 1, (100, 0, 16, 16))]
    dts += [_dt(i, 1, (0, 0, 16, 8), 0.9), _dt(i, 1, (100, 0, 16, 12), 0.8)]
    i = cell("iou_three_fifths", 2)                                # 60 / 100 against whatever float IOU_THRS[2] is
    gts += [_gt(i, 2, (0, 0, 10, 10))]
    dts += [_dt(i, 2, (0, 0, 10, 6), 0.9)]
    i = cell("edge_areas", 3)                                      # areas exactly on both ends of "medium", given and derived
    gts += [_gt(i, 3, (0, 0, 32, 32)), _gt(i, 3, (100, 100, 96, 96)), _gt(i, 3, (300, 0, 50, 50), area=1024.0)]
    dts += [_dt(i, 3, (0, 0, 32, 32), 0.9), _dt(i, 3, (100, 100, 96, 96), 0.8), _dt(i, 3, (300, 0, 50, 50), 0.7), _dt(i, 3, (400, 400, 32, 32), 0.6)]
    return gts, dts, where


@functools.lru_cache(maxsize=None)
def test_set():
    """-> (ground truths, detections, image ids, category ids, the hand-made cells); image 99 and category 4 have no record at all,
    category 5 only ground truths"""
    g1, d1 = generated()
    g2, d2, where = hand_made()
    imgs = sorted({r["image_id"] for r in g1 + d1 + g2 + d2} | {99})
    return g1 + g2, d1 + d2, imgs, list(CATS) + [4, 5], where


test_set.__test__ = False      # a fixture's name, not a test
