"""KITTI result format + AP evaluation (the 3D half: "COCO/KITTI result formats + AP evaluation").

What the reference does after its PointPillars path:
  * pointpillars/src/predict.py:204-262, 331-395 -- lidar boxes -> camera boxes -> image boxes -> KITTI annotation dicts
    (`lidar_boxes_to_prediction`, `predictions_to_kitti_annos` here);
  * pointpillars/src/core/eval_utils.py (what pointpillars/eval.py:149 calls: image-bbox AP only, 11 recall points) and
    pointpillars/eval_gpu/eval.py (the full protocol: bbox / BEV / 3D AP + AOS, 11- and 40-point AP, rotated overlaps from a
    numba-CUDA kernel) -- `get_official_eval_result(..., protocol="ms" | "full")` here.

Protocol (KITTI object benchmark as both files state it): per class and difficulty (min image height 40/25/25 px, max
occlusion 0/1/2, max truncation 0.15/0.3/0.5) ground truth is split into counted / ignored (neighbour class or too hard) /
other; detections below the height limit are ignored.  A first greedy pass (highest score first per ground truth) collects the
scores of all matched detections; 41 score thresholds are picked from them at equally spaced recall; a second pass per
threshold counts TP / FP / FN with the best-overlap assignment, detections matching ignored ground truth or lying in DontCare
regions (image metric only) are not false positives.  precision[i] = max over later thresholds; AP = mean of precision at
recall points 0, 4, ..., 40 (11-point) or 1..40 (R40).  AOS accumulates (1 + cos(delta alpha)) / 2 over true positives.

The rotated BEV intersections come from `det_ops.rotate_iou_gpu_eval` (md_rotate_iou_eval, the HIP counterpart of
eval_gpu/rotate_iou.py:264-340) exactly where the reference calls its CUDA kernel; everything else is host numpy like the
reference's.  Pinning (tests/test_kitti_eval_cpu.py): the "ms" protocol reproduces the reference's own outputs -- result text,
mAP table, 41-point precision rows, clean_data flags, get_thresholds -- on 223 synthetic images (tests/golden/
kitti_eval_vectors.json, written by tests/golden/gen_kitti_eval.py from pointpillars/src/core/eval_utils.py imported with numba's
decorators as identities).  The "full" protocol shares that machinery; its BEV / 3D / AOS parts (eval_gpu/eval.py needs
numba.cuda) are checked against a scalar restatement of the matching rules and hand-computed answers only: parity unpinned there,
as is any run on real KITTI results.  `rows_to_annos` formats the rows that det_ops.kitti_rows (md_kitti_rows) wrote on the device -- the same
filters, clip and alpha for a batch with nothing read back in between -- into the same dicts.  The lidar -> camera -> image box geometry reproduces the reference's box_ops.py outputs (same
golden file); the annotation writer's filter rules (predict.py needs skimage through kitti_common: not importable) are restated.  Reference quirk: eval_utils.get_split_parts has no guard, fewer than 50 images crash it.

Coincident boxes (a property of the reference's rotated overlap, eval_gpu/rotate_iou.py:164-179, kept here): its corner-inside test is a
non-strict fp32 `>=` and its edge-crossing test a strict `>`, so when corners of one box lie on the edges of the other the roundings
decide which vertices the intersection polygon gets.  Measured on the fp32 restatement of that arithmetic, 257 car-sized pairs in
KITTI's range each (tests/rot_eval_contract.py, tests/test_rot_eval_contract_cpu.py): a box against a bit-identical copy of itself
comes out with an IoU below 0.99 -- mostly 0 or about 1/3 -- for 98.8 % of the pairs at arbitrary yaw and for 74.7 % at yaw in
{+-1.57, pi}; only at yaw exactly 0 is it 1.  Equal yaw with one shared edge line: 13.6 % below 0.99 of the true IoU.  One thing is not
kept: for two collinear edges the reference's crossing point is a quotient of two rounding residues (restated literally: intersection
areas up to 672 m2 for cars, IoU from -34.6 to +30.8, for 36 % of such pairs); csrc/rot_eval.h keeps a crossing only if it lies on
both segments, which changes no other pair the tests know.  Evaluating a result set against a bit-identical copy of itself is
therefore not a sanity check this metric supports unless every yaw is 0.  Away from coincidence the kernels are held to a float64
geometric judge (tests/test_rot_eval_gpu.py).

The device path (at the end of this file; include/minddet_hip_kittieval.h): pack_annos lays the annotations of all images out as one flat
set of tensors (PackedEval; with_rows takes the detection half from md_kitti_rows' device rows), eval_class_device runs clean_data, the
overlaps, both matching passes, get_thresholds and the sums over the images as the five md_kitti_eval_* operators and ends in the same
host tail as eval_class; get_official_eval_result(backend="device") selects it.  The host functions above stay as they are: they are the
default and the judge of the device path (tests/test_kitti_eval_device_gpu.py).
"""
import numpy as np

CLASS_NAMES_FULL = ("car", "pedestrian", "cyclist", "van", "person_sitting", "truck")                 # eval_gpu/eval.py:31
CLASS_NAMES_MS = ("car", "pedestrian", "cyclist", "van", "person_sitting", "car", "tractor", "trailer")  # eval_utils.py:98-107
MIN_HEIGHT = (40, 25, 25)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
N_SAMPLE_PTS = 41
_NO_DETECTION = -10000000


# ----------------------------------------------------------------------------- result format (predict.py)
def lidar_to_camera(points, r_rect, velo2cam):
    """box_ops.py:502-510: [.., 3] lidar points -> rectified camera coordinates."""
    pts = np.concatenate([points, np.ones(list(points.shape[:-1]) + [1])], axis=-1)
    return (pts @ (r_rect @ velo2cam).T)[..., :3]


def box_lidar_to_camera(boxes, r_rect, velo2cam):
    """box_ops.py:538-546: (x, y, z, w, l, h, r) lidar -> (x, y, z, l, h, w, r) camera."""
    xyz = lidar_to_camera(boxes[..., 0:3], r_rect, velo2cam)
    w, l, h, r = boxes[..., 3:4], boxes[..., 4:5], boxes[..., 5:6], boxes[..., 6:7]
    return np.concatenate([xyz, l, h, w, r], axis=-1)


def camera_box_corners(boxes):
    """box_ops.py:550-631: camera boxes [N,7] (bottom-centre origin) -> corners [N,8,3] float32."""
    n = boxes.shape[0]
    l, h, w, ry = boxes[:, 3], boxes[:, 4], boxes[:, 5], boxes[:, 6]
    xc = np.stack([l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2], 1).astype(np.float32)
    zc = np.stack([w / 2, -w / 2, -w / 2, w / 2, w / 2, -w / 2, -w / 2, w / 2], 1).astype(np.float32)
    yc = np.zeros((n, 8), np.float32)
    yc[:, 4:8] = -h.reshape(n, 1)
    c, s = np.cos(ry), np.sin(ry)
    zeros, ones = np.zeros(n, np.float32), np.ones(n, np.float32)
    rot = np.transpose(np.array([[c, zeros, -s], [zeros, ones, zeros], [s, zeros, c]]), (2, 0, 1))   # [N,3,3]
    corners = np.matmul(np.stack([xc, yc, zc], 2), rot) + boxes[:, None, 0:3]
    return corners.astype(np.float32)


def camera_boxes_to_image_boxes(boxes, p2):
    """box_ops.py:641-668: project the 8 corners with P2 ([4,4] or [3,4]) and take their bounding rectangle [N,4]."""
    corners = camera_box_corners(boxes).reshape(-1, 3)
    hom = np.hstack((corners, np.ones((corners.shape[0], 1), np.float32)))
    uvw = hom @ np.asarray(p2).T
    uv = (uvw[:, 0:2].T / hom[:, 2]).T.reshape(-1, 8, 2)
    return np.concatenate([uv.min(1), uv.max(1)], axis=1)


def lidar_boxes_to_prediction(boxes_lidar, labels, scores, rect, trv2c, p2, image_idx, dir_labels=None):
    """predict.py:204-262 (`generate_single_sample_dict_old`): selected lidar boxes -> the prediction dict the annotation writer
    consumes.  `dir_labels` applies the direction-classifier flip (:221-236)."""
    if boxes_lidar is None or len(boxes_lidar) == 0:
        return dict(bbox=None, box3d_camera=None, box3d_lidar=None, scores=None, label_preds=None, image_idx=image_idx)
    boxes_lidar = np.array(boxes_lidar, np.float64)
    if dir_labels is not None:
        opp = (boxes_lidar[..., -1] > 0) ^ np.asarray(dir_labels).astype(bool)
        boxes_lidar[..., -1] += np.where(opp, np.pi, 0.0)
    cam = box_lidar_to_camera(boxes_lidar, rect, trv2c)
    return dict(bbox=camera_boxes_to_image_boxes(cam, p2), box3d_camera=cam, box3d_lidar=boxes_lidar, scores=np.asarray(scores),
                label_preds=np.asarray(labels), image_idx=image_idx)


def empty_result_anno():
    """kitti_common.py:439-455"""
    return dict(name=np.array([]), truncated=np.array([]), occluded=np.array([]), alpha=np.array([]), bbox=np.zeros([0, 4]),
                dimensions=np.zeros([0, 3]), location=np.zeros([0, 3]), rotation_y=np.array([]), score=np.array([]))


def predictions_to_kitti_annos(predictions, batch_image_shape, class_names, center_limit_range=None, lidar_input=False):
    """predict.py:331-395 (`predict_kitti_to_anno`): drop boxes outside the image / the centre range, clip the image box, write
    (name, truncated 0, occluded 0, alpha, bbox, dimensions, location, rotation_y, score) + image_idx."""
    annos = []
    for i, pred in enumerate(predictions):
        image_shape = np.asarray(batch_image_shape[i])
        rows = {k: [] for k in ("name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score")}
        if pred["bbox"] is not None:
            for box, box_lidar, bbox, score, label in zip(pred["box3d_camera"], pred["box3d_lidar"], pred["bbox"], pred["scores"],
                                                          pred["label_preds"]):
                bbox = np.array(bbox, np.float64)
                if not lidar_input:
                    if bbox[0] > image_shape[1] or bbox[1] > image_shape[0] or bbox[2] < 0 or bbox[3] < 0:
                        continue
                if center_limit_range is not None:
                    lim = np.asarray(center_limit_range)
                    if np.any(box_lidar[:3] < lim[:3]) or np.any(box_lidar[:3] > lim[3:]):
                        continue
                bbox[2:] = np.minimum(bbox[2:], image_shape[::-1])
                bbox[:2] = np.maximum(bbox[:2], [0, 0])
                rows["name"].append(class_names[int(label)])
                rows["truncated"].append(0.0)
                rows["occluded"].append(0)
                rows["alpha"].append(-np.arctan2(-box_lidar[1], box_lidar[0]) + box[6])
                rows["bbox"].append(bbox)
                rows["dimensions"].append(box[3:6])
                rows["location"].append(box[:3])
                rows["rotation_y"].append(box[6])
                rows["score"].append(score)
        anno = {k: np.stack(v) for k, v in rows.items()} if rows["name"] else empty_result_anno()
        anno["image_idx"] = np.array([pred["image_idx"]] * anno["name"].shape[0], dtype=np.int64)
        annos.append(anno)
    return annos


def rows_to_annos(rows, src, count, dets, class_names, image_idx):
    """The result rows of det_ops.kitti_rows / PointPillarsKITTIPoints.forward_kitti ([B,M,14]: alpha, bbox, dimensions l h w, location,
    rotation_y, score, label; src [B,M]; count [B]; device tensors or arrays) -> the annotation dicts predictions_to_kitti_annos returns,
    one per sample.  Host formatting only: the filters, the clip and alpha were applied on the device; this adds the names,
    truncated 0, occluded 0 and image_idx.  `dets` (the detections the rows came from) is not read: src says which row each one was."""
    rows, src, count = (np.asarray(t.cpu().numpy() if hasattr(t, "cpu") else t) for t in (rows, src, count))
    annos = []
    for b in range(rows.shape[0]):
        n = int(count[b])
        if n == 0:
            anno = empty_result_anno()
        else:
            r = rows[b, :n].astype(np.float64)
            anno = dict(name=np.array([class_names[int(k)] for k in r[:, 13]]), truncated=np.zeros(n), occluded=np.zeros(n, np.int64),
                        alpha=r[:, 0], bbox=r[:, 1:5], dimensions=r[:, 5:8], location=r[:, 8:11], rotation_y=r[:, 11], score=r[:, 12])
        anno["image_idx"] = np.array([image_idx[b]] * n, dtype=np.int64)
        annos.append(anno)
    return annos


def kitti_result_lines(anno):
    """One KITTI label-file line per detection: name truncated occluded alpha bbox(4) dimensions as (h, w, l) location(3)
    rotation_y score -- `dimensions` is stored (l, h, w) as above (kitti_common.py convention)."""
    lines = []
    for i in range(len(anno["name"])):
        l, h, w = anno["dimensions"][i]
        vals = [anno["alpha"][i], *anno["bbox"][i], h, w, l, *anno["location"][i], anno["rotation_y"][i], anno["score"][i]]
        lines.append(f"{anno['name'][i]} {float(anno['truncated'][i]):.2f} {int(anno['occluded'][i])} " + " ".join(f"{float(v):.4f}" for v in vals))
    return lines


# ----------------------------------------------------------------------------- overlaps
def image_box_overlap(boxes, query_boxes, criterion=-1):
    """eval_gpu/eval.py:91-121: [N,4] x [K,4] image boxes; criterion -1 IoU, 0 / boxes area, 1 / query area, else intersection."""
    boxes, query_boxes = np.asarray(boxes, np.float64).reshape(-1, 4), np.asarray(query_boxes, np.float64).reshape(-1, 4)
    iw = np.minimum(boxes[:, None, 2], query_boxes[None, :, 2]) - np.maximum(boxes[:, None, 0], query_boxes[None, :, 0])
    ih = np.minimum(boxes[:, None, 3], query_boxes[None, :, 3]) - np.maximum(boxes[:, None, 1], query_boxes[None, :, 1])
    ok = (iw > 0) & (ih > 0)
    inter = np.where(ok, iw * ih, 0.0)
    a = ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]))[:, None]
    q = ((query_boxes[:, 2] - query_boxes[:, 0]) * (query_boxes[:, 3] - query_boxes[:, 1]))[None, :]
    if criterion == -1:
        ua = a + q - inter
    elif criterion == 0:
        ua = a + 0 * q
    elif criterion == 1:
        ua = q + 0 * a
    else:
        ua = np.ones_like(inter)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ok, inter / ua, 0.0)


def _device_rotate_iou(boxes, query_boxes, criterion):
    import torch

    from . import det_ops
    dev = "cuda:0"
    return det_ops.rotate_iou_gpu_eval(torch.from_numpy(np.ascontiguousarray(boxes, np.float32)).to(dev),
                                       torch.from_numpy(np.ascontiguousarray(query_boxes, np.float32)).to(dev), criterion).cpu().numpy()


def bev_box_overlap(boxes, qboxes, criterion=-1, rotate_iou=None):
    """eval_gpu/eval.py:124-126: [N,5] x [K,5] (x, z, l, w, ry)."""
    if len(boxes) == 0 or len(qboxes) == 0:
        return np.zeros((len(boxes), len(qboxes)))
    return np.asarray((rotate_iou or _device_rotate_iou)(boxes, qboxes, criterion), np.float64)


def d3_box_overlap(boxes, qboxes, criterion=-1, rotate_iou=None):
    """eval_gpu/eval.py:129-162: camera boxes [N,7] (x, y, z, l, h, w, ry), y = bottom face, -y up: BEV intersection area x
    overlap of the [y - h, y] intervals over the volume union."""
    if len(boxes) == 0 or len(qboxes) == 0:
        return np.zeros((len(boxes), len(qboxes)))
    rinc = np.asarray((rotate_iou or _device_rotate_iou)(boxes[:, [0, 2, 3, 5, 6]], qboxes[:, [0, 2, 3, 5, 6]], 2), np.float64)
    ih = np.minimum(boxes[:, None, 1], qboxes[None, :, 1]) - np.maximum(boxes[:, None, 1] - boxes[:, None, 4], qboxes[None, :, 1] - qboxes[None, :, 4])
    v1 = (boxes[:, 3] * boxes[:, 4] * boxes[:, 5])[:, None]
    v2 = (qboxes[:, 3] * qboxes[:, 4] * qboxes[:, 5])[None, :]
    inc = ih * rinc
    ok = (rinc > 0) & (ih > 0)
    ua = {-1: v1 + v2 - inc, 0: v1 + 0 * v2, 1: v2 + 0 * v1}.get(criterion, inc)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(ok, inc / ua, 0.0)
    return np.where(rinc > 0, out, rinc)          # cells without BEV intersection keep the kernel's value (0)


# ----------------------------------------------------------------------------- matching
def get_thresholds(scores, num_gt, num_sample_pts=N_SAMPLE_PTS):
    """eval_gpu/eval.py:9-27: scores of matched detections -> the thresholds at (about) equally spaced recall."""
    scores = np.sort(np.asarray(scores, np.float64))[::-1]
    current_recall, thresholds = 0.0, []
    for i, score in enumerate(scores):
        l_recall = (i + 1) / num_gt
        r_recall = (i + 2) / num_gt if i < len(scores) - 1 else l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < len(scores) - 1:
            continue
        thresholds.append(score)
        current_recall += 1 / (num_sample_pts - 1.0)
    return thresholds


def clean_data(gt_anno, dt_anno, current_class, difficulty, class_names=CLASS_NAMES_FULL):
    """eval_gpu/eval.py:30-87 / eval_utils.py:36-115 -> (num_valid_gt, ignored_gt, ignored_dt, dc_bboxes); flags 0 counted,
    1 ignored, -1 other class."""
    cur = class_names[current_class].lower()
    ignored_gt, ignored_dt, dc = [], [], []
    num_valid = 0
    for i in range(len(gt_anno["name"])):
        bbox = gt_anno["bbox"][i]
        name = str(gt_anno["name"][i]).lower()
        height = bbox[3] - bbox[1]
        if class_names is CLASS_NAMES_MS:
            height = abs(height)                      # eval_utils.py:49 takes the magnitude, eval_gpu/eval.py:44 does not
        if name == cur:
            valid = 1
        elif (cur == "pedestrian" and name == "person_sitting") or (cur == "car" and name == "van"):
            valid = 0
        else:
            valid = -1
        ignore = (gt_anno["occluded"][i] > MAX_OCCLUSION[difficulty] or gt_anno["truncated"][i] > MAX_TRUNCATION[difficulty]
                  or height <= MIN_HEIGHT[difficulty])
        if valid == 1 and not ignore:
            ignored_gt.append(0)
            num_valid += 1
        elif valid == 0 or (ignore and valid == 1):
            ignored_gt.append(1)
        else:
            ignored_gt.append(-1)
        if gt_anno["name"][i] == "DontCare":
            dc.append(bbox)
    for i in range(len(dt_anno["name"])):
        height = abs(dt_anno["bbox"][i, 3] - dt_anno["bbox"][i, 1])
        if height < MIN_HEIGHT[difficulty]:
            ignored_dt.append(1)
        elif str(dt_anno["name"][i]).lower() == cur:
            ignored_dt.append(0)
        else:
            ignored_dt.append(-1)
    return num_valid, ignored_gt, ignored_dt, dc


def compute_statistics(overlaps, gt_datas, dt_datas, ignored_gt, ignored_det, dc_bboxes, metric, min_overlap, thresh=0.0,
                       compute_fp=False, compute_aos=False):
    """eval_gpu/eval.py:166-297.  overlaps [D,G]; gt_datas [G,5] (bbox, alpha); dt_datas [D,6] (bbox, alpha, score).
    The per-ground-truth scan over detections is evaluated with array operations; the outcome per ground truth is the one the
    reference's sequential scan reaches: without compute_fp the highest-scoring candidate (first on ties); with compute_fp the
    counted candidate of largest overlap (first on ties), else the first ignored candidate.
    -> (tp, fp, fn, similarity, matched scores)."""
    ignored_gt, ignored_det = np.asarray(ignored_gt), np.asarray(ignored_det)
    D, G = dt_datas.shape[0], gt_datas.shape[0]
    dt_scores, dt_alphas, gt_alphas = dt_datas[:, -1], dt_datas[:, 4], gt_datas[:, 4]
    assigned = np.zeros(D, bool)
    below = (dt_scores < thresh) if compute_fp else np.zeros(D, bool)
    usable = (ignored_det != -1) & ~below
    tp = fp = fn = 0
    similarity = 0
    matched_scores, delta = [], []
    for i in range(G):
        if ignored_gt[i] == -1:
            continue
        cand = usable & ~assigned & (overlaps[:, i] > min_overlap) if D else np.zeros(0, bool)
        det_idx = -1
        if not compute_fp:
            if cand.any():
                idx = np.flatnonzero(cand)
                det_idx = int(idx[np.argmax(dt_scores[idx])])
        else:
            counted = cand & (ignored_det == 0)
            if counted.any():
                idx = np.flatnonzero(counted)
                det_idx = int(idx[np.argmax(overlaps[idx, i])])
            else:
                ign = cand & (ignored_det == 1)
                if ign.any():
                    det_idx = int(np.flatnonzero(ign)[0])
        if det_idx < 0:
            if ignored_gt[i] == 0:
                fn += 1
        elif ignored_gt[i] == 1 or ignored_det[det_idx] == 1:
            assigned[det_idx] = True
        else:
            tp += 1
            matched_scores.append(dt_scores[det_idx])
            if compute_aos:
                delta.append(gt_alphas[i] - dt_alphas[det_idx])
            assigned[det_idx] = True
    if compute_fp:
        fp = int(np.sum(~(assigned | (ignored_det == -1) | (ignored_det == 1) | below)))
        nstuff = 0
        if metric == 0 and len(dc_bboxes):
            ov = image_box_overlap(dt_datas[:, :4], dc_bboxes, 0)
            for i in range(len(dc_bboxes)):
                hit = ~assigned & (ignored_det == 0) & ~below & (ov[:, i] > min_overlap)
                nstuff += int(hit.sum())
                assigned |= hit
        fp -= nstuff
        if compute_aos:
            similarity = float(np.sum((1.0 + np.cos(np.asarray(delta, np.float64))) / 2.0)) if (tp > 0 or fp > 0) else -1
    return tp, fp, fn, similarity, np.asarray(matched_scores, np.float64)


def _boxes_of(annos, metric):
    if metric == 0:
        return [np.asarray(a["bbox"], np.float64).reshape(-1, 4) for a in annos]
    out = []
    for a in annos:
        loc, dims, rot = (np.asarray(a[k], np.float64) for k in ("location", "dimensions", "rotation_y"))
        loc, dims = loc.reshape(-1, 3), dims.reshape(-1, 3)
        if metric == 1:
            loc, dims = loc[:, [0, 2]], dims[:, [0, 2]]
        out.append(np.concatenate([loc, dims, rot.reshape(-1, 1)], axis=1))
    return out


def calculate_overlaps(gt_annos, dt_annos, metric, rotate_iou=None):
    """eval_gpu/eval.py:366-437 per image (the reference batches images into parts for its GPU kernel and slices the diagonal
    blocks back out; the blocks are the same).  -> list of [D_i, G_i] (detections x ground truth, the orientation eval_class
    uses: it calls calculate_iou_partly(dt_annos, gt_annos), :511)."""
    fn = {0: lambda b, q: image_box_overlap(b, q), 1: lambda b, q: bev_box_overlap(b, q, -1, rotate_iou),
          2: lambda b, q: d3_box_overlap(b, q, -1, rotate_iou)}.get(metric)
    if fn is None:
        raise ValueError("unknown metric")
    return [fn(d, g) for d, g in zip(_boxes_of(dt_annos, metric), _boxes_of(gt_annos, metric))]


def _curves_from_counts(pr, precision, recall, aos=None):
    """The tail of eval_class (eval_gpu/eval.py:577-594) for one (class, difficulty, overlap level): pr [nt,4] (tp, fp, fn, similarity
    summed over the images, one row per threshold) -> the 41-long zero rows precision / recall / aos filled in place: the divisions,
    then the right-to-left envelope.  eval_class and eval_class_device both end here."""
    nt = len(pr)
    with np.errstate(divide="ignore", invalid="ignore"):
        recall[:nt] = pr[:, 0] / (pr[:, 0] + pr[:, 2])
        precision[:nt] = pr[:, 0] / (pr[:, 0] + pr[:, 1])
        if aos is not None:
            aos[:nt] = pr[:, 3] / (pr[:, 0] + pr[:, 1])
    for i in range(nt):      # the envelope runs over the whole 41-long row (zeros past nt), as in :590-594
        precision[i] = np.max(precision[i:])
        recall[i] = np.max(recall[i:])
        if aos is not None:
            aos[i] = np.max(aos[i:])


def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False,
               class_names=CLASS_NAMES_FULL, rotate_iou=None):
    """eval_gpu/eval.py:483-599 -> {"recall", "precision", "orientation"}: [class, difficulty, min_overlap, 41]."""
    if len(gt_annos) != len(dt_annos):
        raise ValueError("gt_annos and dt_annos must pair up image by image")
    overlaps = calculate_overlaps(gt_annos, dt_annos, metric, rotate_iou)
    shape = [len(current_classes), len(difficultys), len(min_overlaps), N_SAMPLE_PTS]
    precision, recall, aos = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    for m, cls in enumerate(current_classes):
        for n, difficulty in enumerate(difficultys):
            gt_datas, dt_datas, ign_gts, ign_dts, dcs = [], [], [], [], []
            total_valid = 0
            for g, d in zip(gt_annos, dt_annos):
                nv, ig, idt, dc = clean_data(g, d, cls, difficulty, class_names)
                total_valid += nv
                ign_gts.append(np.array(ig, np.int64))
                ign_dts.append(np.array(idt, np.int64))
                dcs.append(np.stack(dc, 0).astype(np.float64) if dc else np.zeros((0, 4)))
                gt_datas.append(np.concatenate([np.asarray(g["bbox"], np.float64).reshape(-1, 4), np.asarray(g["alpha"], np.float64).reshape(-1, 1)], 1))
                dt_datas.append(np.concatenate([np.asarray(d["bbox"], np.float64).reshape(-1, 4), np.asarray(d["alpha"], np.float64).reshape(-1, 1),
                                                np.asarray(d["score"], np.float64).reshape(-1, 1)], 1))
            for k, min_overlap in enumerate(min_overlaps[:, metric, m]):
                scores = [compute_statistics(overlaps[i], gt_datas[i], dt_datas[i], ign_gts[i], ign_dts[i], dcs[i], metric, min_overlap, 0.0, False)[4]
                          for i in range(len(gt_annos))]
                thresholds = np.array(get_thresholds(np.concatenate(scores) if scores else np.zeros(0), total_valid))
                pr = np.zeros([len(thresholds), 4])
                for i in range(len(gt_annos)):
                    for t, thresh in enumerate(thresholds):
                        tp, fp, fn, sim, _ = compute_statistics(overlaps[i], gt_datas[i], dt_datas[i], ign_gts[i], ign_dts[i], dcs[i], metric,
                                                                min_overlap, thresh, True, compute_aos)
                        pr[t, 0] += tp
                        pr[t, 1] += fp
                        pr[t, 2] += fn
                        if sim != -1:
                            pr[t, 3] += sim
                _curves_from_counts(pr, precision[m, n, k], recall[m, n, k], aos[m, n, k] if compute_aos else None)
    return {"recall": recall, "precision": precision, "orientation": aos}


def get_map(prec):
    """11-point AP (eval_gpu/eval.py:602-606, eval_utils.py:609-614)."""
    return sum(prec[..., i] for i in range(0, prec.shape[-1], 4)) / 11 * 100


def get_map_r40(prec):
    """40-point AP (eval_gpu/eval.py:609-613)."""
    return sum(prec[..., i] for i in range(1, prec.shape[-1])) / 40 * 100


_MIN_OVERLAPS_FULL = np.stack([np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.7]] * 3),
                               np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5]])], 0)
_MIN_OVERLAPS_MS = np.array([[[0.7, 0.5, 0.5, 0.7, 0.5, 0.7, 0.7, 0.7]] * 3])
_NAMES_FULL = {0: "Car", 1: "Pedestrian", 2: "Cyclist", 3: "Van", 4: "Person_sitting", 5: "Truck"}
_NAMES_MS = {0: "Car", 1: "Pedestrian", 2: "Cyclist", 3: "Van", 4: "Person_sitting", 5: "car", 6: "tractor", 7: "trailer"}


def _wants_aos(dt_annos):
    """eval_gpu/eval.py:738-744: the first non-empty detection annotation decides"""
    for anno in dt_annos:
        if anno["alpha"].shape[0] != 0:
            return bool(anno["alpha"][0] != -10)
    return False


def get_official_eval_result(gt_annos, dt_annos, current_classes, protocol="full", difficultys=(0, 1, 2), rotate_iou=None, backend="host",
                             packed=None):
    """protocol "ms": eval_utils.py:645-702 (what pointpillars/eval.py prints: image-bbox AP, 11 points) -> (text, map_bbox
    [class, difficulty, 1]).  protocol "full": eval_gpu/eval.py:697-885 -> (text, dict of the *_R40 entries); AOS is computed
    when the first non-empty detection annotation carries a real alpha (!= -10), :738-744.
    backend "host": eval_class, numpy loops around md_rotate_iou_eval.  backend "device": the annotations are packed once
    (pack_annos; or `packed`, a PackedEval made earlier, e.g. by PackedEval.with_rows, and then dt_annos is not read) and every metric
    runs through eval_class_device: the md_kitti_eval_* operators, with the divisions and the envelope on the host as before."""
    if backend not in ("host", "device"):
        raise ValueError(f"backend is 'host' or 'device', got {backend!r}")
    if packed is not None and backend != "device":
        raise ValueError("a PackedEval is evaluated by backend='device'")
    ms = protocol == "ms"
    names, table = (_NAMES_MS, _MIN_OVERLAPS_MS) if ms else (_NAMES_FULL, _MIN_OVERLAPS_FULL)
    to_class = {v: k for k, v in names.items()}
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    classes = [to_class[c] if isinstance(c, str) else c for c in current_classes]
    min_overlaps = table[:, :, classes]
    cn = CLASS_NAMES_MS if ms else CLASS_NAMES_FULL
    if backend == "device":
        if packed is None:
            packed = pack_annos(gt_annos, dt_annos, cn)
        elif tuple(packed.class_names) != tuple(cn):
            raise ValueError(f"the PackedEval was made for the class table {packed.class_names}, protocol {protocol!r} takes {cn}")

        def run(metric, diffs, aos):
            return eval_class_device(packed, classes, diffs, metric, min_overlaps, aos)
    else:
        def run(metric, diffs, aos):
            return eval_class(gt_annos, dt_annos, classes, diffs, metric, min_overlaps, aos, cn, rotate_iou)
    if ms:
        ret = run(0, difficultys, False)
        map_bbox = get_map(ret["precision"])
        text = "        Easy   Mod    Hard\n"
        for j, c in enumerate(classes):
            for i in range(min_overlaps.shape[0]):
                text += f"{names[c]} " + "AP@{:.2f}, {:.2f}, {:.2f}:".format(*min_overlaps[i, :, j]) + "\n"
                text += f"bbox AP: {map_bbox[j, 0, i]: .2f}, {map_bbox[j, 1, i]: .2f}, {map_bbox[j, 2, i]: .2f}\n"
        return text, map_bbox
    compute_aos = _wants_aos(dt_annos) if packed is None else packed.compute_aos
    res = {}
    for metric, key in ((0, "bbox"), (1, "bev"), (2, "3d")):
        ret = run(metric, (0, 1, 2), compute_aos and metric == 0)
        res[key] = (get_map(ret["precision"]), get_map_r40(ret["precision"]))
        if metric == 0 and compute_aos:
            res["aos"] = (get_map(ret["orientation"]), get_map_r40(ret["orientation"]))
    text, out = "", {}
    for j, c in enumerate(classes):
        for i in range(min_overlaps.shape[0]):
            for r40 in (0, 1):
                text += f"{names[c]} " + ("AP_R40" if r40 else "AP") + "@{: .2f}, {: .2f}, {: .2f}:".format(*min_overlaps[i, :, j]) + "\n"
                for key in ("bbox", "bev", "3d"):
                    v = res[key][r40]
                    text += f"{key} AP: {v[j, 0, i]: .4f}, {v[j, 1, i]: .4f}, {v[j, 2, i]: .4f}\n"
                if compute_aos:
                    v = res["aos"][r40]
                    text += f"aos AP: {v[j, 0, i]: .2f}, {v[j, 1, i]: .2f}, {v[j, 2, i]: .2f}\n"
            if i == 0:
                for key, tag in (("3d", "3d"), ("bev", "bev"), ("bbox", "image")) + ((("aos", "aos"),) if compute_aos else ()):
                    v = res[key][1]
                    for d, dn in enumerate(("easy", "moderate", "hard")):
                        out[f"{names[c]}_{tag}/{dn}_R40"] = float(v[j, d, 0])
    return text, out


# ----------------------------------------------------------------------------- the device path (include/minddet_hip_kittieval.h)
MAX_DETS, MAX_GTS, MAX_IMAGES, MAX_CLASSES, MAX_LEVELS = 512, 512, 65536, 8, 4     # the MD_KEVAL_MAX_* of the header


def _valid_codes(names, class_names):
    """[Cn, n] uint8: 1 + the `valid` of clean_data for class c by index in class_names (2 the class, 1 its neighbour class, 0 other)"""
    out = np.zeros((len(class_names), len(names)), np.uint8)
    for c, cur in enumerate(class_names):
        cur = cur.lower()
        for i, name in enumerate(names):
            name = str(name).lower()
            if name == cur:
                out[c, i] = 2
            elif (cur == "pedestrian" and name == "person_sitting") or (cur == "car" and name == "van"):
                out[c, i] = 1
    return out


class PackedEval:
    """Annotations of I images as one flat set of tensors, the operands of the md_kitti_eval_* operators (the layout is stated in
    include/minddet_hip_kittieval.h).  Names stay on the host: they arrive as gt_valid / gt_dc / dt_same codes per class of
    `class_names`.  Made by pack_annos; with_rows replaces the detection half by device rows.  Host-side facts: I, gt_counts [I],
    pairs (the length the overlap tensor takes, >= ov_off[I]), compute_aos, abs_gt_height (the "ms" table's rule)."""
    GT = ("gt_box", "gt_alpha", "gt_occ", "gt_trunc", "gt_dc", "gt_valid", "gt_cam")
    DT = ("dt_box", "dt_alpha", "dt_score", "dt_same", "dt_cam")

    def __init__(self, class_names, device):
        self.class_names, self.device = tuple(class_names), device
        self.abs_gt_height = self.class_names == CLASS_NAMES_MS
        self.gt_cam = self.dt_cam = self.dt_off = None
        self.compute_aos = False

    def with_rows(self, rows, count, class_names):
        """The detection half from the device tensors det_ops.kitti_rows / forward_kitti return: rows [I,M,14] f32 (alpha, bbox,
        dimensions l h w, location, rotation_y, score, label), count [I]; class_names: the detector's label names.  fp32 widened to
        float64, label -> class through a small device table, offsets from a device scan of count; nothing is copied to the host.
        The detection tensors have I M rows, the first dt_off[I] of them are the detections (what pack_annos(rows_to_annos(...)) holds),
        the rest is zero; the overlap tensor takes sum G_i M elements.  compute_aos is set: the rows carry a real alpha."""
        import torch

        if rows.dim() != 3 or rows.shape[2] != 14 or rows.shape[0] != self.I or tuple(count.shape) != (self.I,):
            raise ValueError(f"with_rows: rows are [{self.I}, M, 14] and count [{self.I}], got {tuple(rows.shape)} and {tuple(count.shape)}")
        B, M = rows.shape[:2]
        if M > MAX_DETS:
            raise ValueError(f"with_rows: at most {MAX_DETS} detections per image, got {M}")
        pairs = int(self.gt_counts.sum()) * M
        if pairs >= 1 << 31:
            raise ValueError("with_rows: 2^31 or more overlap pairs")
        dev = rows.device
        out = PackedEval(self.class_names, dev)
        for k in ("I", "gt_counts", "gt_off") + self.GT:
            setattr(out, k, getattr(self, k))
        cnt = count.to(torch.int64).clamp(0, M)
        off = torch.zeros((B + 1,), dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(cnt, 0)
        j = torch.arange(B * M, dtype=torch.int64, device=dev)
        b = torch.searchsorted(off[1:].contiguous(), j, right=True).clamp(max=max(B - 1, 0))
        valid = j < off[B]
        src = torch.where(valid, b * M + (j - off[b]), torch.zeros_like(j)) if B * M else j
        r = torch.where(valid[:, None], rows.reshape(B * M, 14)[src].to(torch.float64), torch.zeros((), dtype=torch.float64, device=dev))
        table = torch.from_numpy(np.array([[n.lower() == c.lower() for n in class_names] for c in self.class_names], np.uint8).reshape(
            len(self.class_names), len(class_names))).to(dev)
        label = r[:, 13].to(torch.int64).clamp(0, max(len(class_names) - 1, 0))
        out.dt_off = off.to(torch.int32)
        out.dt_alpha, out.dt_box, out.dt_score = r[:, 0].contiguous(), r[:, 1:5].contiguous(), r[:, 12].contiguous()
        out.dt_cam = torch.cat([r[:, 8:11], r[:, 5:8], r[:, 11:12]], 1).contiguous()
        out.dt_same = (table[:, label] * valid.to(torch.uint8)[None]).contiguous()
        ov_off = torch.zeros((B + 1,), dtype=torch.int64, device=dev)
        ov_off[1:] = torch.cumsum(torch.from_numpy(self.gt_counts.astype(np.int64)).to(dev) * cnt, 0)
        out.ov_off, out.pairs, out.compute_aos = ov_off, pairs, True
        return out


def pack_annos(gt_annos, dt_annos, class_names=CLASS_NAMES_FULL, device="cuda"):
    """Annotation dicts of I images -> PackedEval.  dt_annos None packs the ground truth alone (for PackedEval.with_rows).
    Annotations without location / dimensions / rotation_y pack without the *_cam tensors (metrics 1 and 2 then raise ValueError).
    Beyond the limits of include/minddet_hip_kittieval.h: ValueError."""
    import torch

    I = len(gt_annos)
    if dt_annos is not None and len(dt_annos) != I:
        raise ValueError("gt_annos and dt_annos must pair up image by image")
    if I > MAX_IMAGES or len(class_names) > MAX_CLASSES or len(class_names) < 1:
        raise ValueError(f"pack_annos: at most {MAX_IMAGES} images and 1 to {MAX_CLASSES} classes")
    p = PackedEval(class_names, device)
    p.I = I

    def put(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(device)

    def col(annos, key, width=None):
        parts = [np.asarray(a[key], np.float64).reshape((-1, width) if width else (-1,)) for a in annos]
        return np.concatenate(parts, 0) if parts else np.zeros((0, width) if width else (0,))

    def cam(annos):
        if not all(k in a for a in annos for k in ("location", "dimensions", "rotation_y")):
            return None
        return np.concatenate([col(annos, "location", 3), col(annos, "dimensions", 3), col(annos, "rotation_y").reshape(-1, 1)], 1)

    def offsets(annos, limit, what):
        n = np.array([len(a["name"]) for a in annos], np.int64)
        if len(n) and n.max() > limit:
            raise ValueError(f"pack_annos: at most {limit} {what} per image, got {int(n.max())}")
        return n, np.concatenate([[0], np.cumsum(n)])

    g, g_off = offsets(gt_annos, MAX_GTS, "ground truths")
    names = [str(n) for a in gt_annos for n in a["name"]]
    p.gt_counts = g
    p.gt_off = put(g_off, np.int32)
    p.gt_box, p.gt_alpha, p.gt_trunc = put(col(gt_annos, "bbox", 4), np.float64), put(col(gt_annos, "alpha"), np.float64), put(col(gt_annos, "truncated"), np.float64)
    p.gt_occ = put(col(gt_annos, "occluded"), np.int32)
    p.gt_dc = put(np.array([n == "DontCare" for n in names], np.uint8).reshape(-1), np.uint8)
    p.gt_valid = put(_valid_codes(names, class_names), np.uint8)
    c = cam(gt_annos)
    p.gt_cam = None if c is None else put(c, np.float64)
    if dt_annos is None:
        return p
    d, d_off = offsets(dt_annos, MAX_DETS, "detections")
    ov = np.concatenate([[0], np.cumsum(g * d)])
    if ov[-1] >= 1 << 31:
        raise ValueError("pack_annos: 2^31 or more overlap pairs")
    dnames = [str(n).lower() for a in dt_annos for n in a["name"]]
    p.dt_off, p.ov_off, p.pairs = put(d_off, np.int32), put(ov, np.int64), int(ov[-1])
    p.dt_box, p.dt_alpha, p.dt_score = put(col(dt_annos, "bbox", 4), np.float64), put(col(dt_annos, "alpha"), np.float64), put(col(dt_annos, "score"), np.float64)
    p.dt_same = put(np.array([[n == cn.lower() for n in dnames] for cn in class_names], np.uint8).reshape(len(class_names), len(dnames)), np.uint8)
    c = cam(dt_annos)
    p.dt_cam = None if c is None else put(c, np.float64)
    p.compute_aos = _wants_aos(dt_annos)
    return p


def device_tables(packed, current_classes, metric, min_overlaps, compute_aos=False):
    """The five md_kitti_eval_* calls on a PackedEval -> dict of device tensors: ign_gt, ign_dt, num_valid, ov, matched, thresholds,
    nthresh, img_counts, img_sim, pr_counts, pr_sim, each [class of current_classes, 3 difficulties, overlap level, ...].  Nothing is
    read back here."""
    import torch

    from . import det_ops
    if metric not in (0, 1, 2):
        raise ValueError("unknown metric")
    if metric != 0 and (packed.gt_cam is None or packed.dt_cam is None):
        raise ValueError("metrics 1 and 2 take location, dimensions and rotation_y, which these annotations lack")
    if packed.dt_off is None:
        raise ValueError("this PackedEval holds ground truth only: pack detections, or use with_rows")
    cls = [int(c) for c in current_classes]
    mo = np.asarray(min_overlaps, np.float64)[:, metric, :]                 # [K, class]
    if mo.shape[1] != len(cls) or not cls or max(cls) >= len(packed.class_names) or min(cls) < 0:
        raise ValueError("min_overlaps is [K, 3, len(current_classes)] and the classes index the pack's class table")
    if mo.shape[0] > MAX_LEVELS:
        raise ValueError(f"at most {MAX_LEVELS} overlap levels")
    dev = packed.gt_box.device
    idx = torch.tensor(cls, dtype=torch.int64, device=dev)
    min_overlap = torch.from_numpy(np.ascontiguousarray(mo.T)).to(dev)
    t = {}
    t["ign_gt"], t["ign_dt"], t["num_valid"] = det_ops.kitti_eval_flags(packed.gt_box, packed.gt_occ, packed.gt_trunc, packed.gt_valid[idx],
                                                                        packed.dt_box, packed.dt_same[idx], packed.abs_gt_height)
    gt, dt = (packed.gt_box, packed.dt_box) if metric == 0 else (packed.gt_cam, packed.dt_cam)
    t["ov"] = det_ops.kitti_eval_overlaps(packed.gt_off, packed.dt_off, packed.ov_off, gt, dt, metric, packed.pairs)
    offs = (packed.gt_off, packed.dt_off, packed.ov_off, min_overlap)
    t["matched"] = det_ops.kitti_eval_match(t["ov"], t["ign_gt"], t["ign_dt"], packed.dt_score, *offs)
    ordered = torch.sort(t["matched"], dim=-1, descending=True).values      # plumbing: equal values are interchangeable
    t["thresholds"], t["nthresh"] = det_ops.kitti_eval_thresholds(ordered, t["num_valid"])
    t["img_counts"], t["img_sim"], t["pr_counts"], t["pr_sim"] = det_ops.kitti_eval_stats(
        t["ov"], t["ign_gt"], t["ign_dt"], packed.dt_score, *offs, t["thresholds"], t["nthresh"], packed.gt_box, packed.gt_dc, packed.dt_box,
        packed.gt_alpha, packed.dt_alpha, metric, compute_aos)
    return t


def eval_class_device(packed, current_classes, difficultys, metric, min_overlaps, compute_aos=False):
    """eval_class on the device path: the count tables come from device_tables (one read of [class, 3, K, 41] counts at the end), the
    divisions and the envelope from the helper eval_class ends in.  Same dict, shapes and NaN conventions as eval_class."""
    t = device_tables(packed, current_classes, metric, min_overlaps, compute_aos)
    counts, sim, nth = t["pr_counts"].cpu().numpy().astype(np.float64), t["pr_sim"].cpu().numpy(), t["nthresh"].cpu().numpy()
    shape = [len(current_classes), len(difficultys), counts.shape[2], N_SAMPLE_PTS]
    precision, recall, aos = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    for m in range(shape[0]):
        for n, difficulty in enumerate(difficultys):
            for k in range(shape[2]):
                nt = int(nth[m, difficulty, k])
                pr = np.concatenate([counts[m, difficulty, k, :nt], sim[m, difficulty, k, :nt, None]], 1)
                _curves_from_counts(pr, precision[m, n, k], recall[m, n, k], aos[m, n, k] if compute_aos else None)
    return {"recall": recall, "precision": precision, "orientation": aos}
