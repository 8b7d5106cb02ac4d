"""COCO result format + bbox AP without pycocotools ("the step after the path").

* `convert_eval_format` mirrors minddet/models/centernet/src/post_process.py:64-89: per-class detections -> COCO result
  records (xywh, 2-decimal floats exactly as the reference's `to_float`).
* `dets_to_coco` does the same from the fixed-shape device output `dets [B,max_det,6]` + `count [B]`.
* `COCOBboxEval` restates the published COCOeval bbox protocol the reference calls at centernet/eval.py:181-187
  (`COCOeval(coco, coco_dets, "bbox"); evaluate(); accumulate(); summarize()`): IoU thresholds 0.50:0.05:0.95, 101 recall
  points, area ranges all / small / medium / large, maxDets 1 / 10 / 100, crowd ground truth matched many-to-one with
  IoU = intersection / detection area, ignored ground truth (crowd or outside the area range) sorted last and never
  counted.  pycocotools is not installable here, so the evaluator is checked against hand-computed known answers
  (tests/test_coco_eval_cpu.py): parity with pycocotools itself is unpinned.

Host-side numpy, like the reference's own evaluation step (pycocotools runs on the CPU there too).

The device path (at the end of this file; include/minddet_hip_cocoeval.h): pack_coco lays the records out as flat device tensors per
(image, category) cell, PackedCoco.add_dets takes a detector's (dets, count) straight from the device (md_coco_eval_rows: to_float and
the grouping, no host read), and COCOBboxEval.evaluate(backend="device") / COCOBboxEval.from_packed fill precision and recall from
md_coco_eval_match and md_coco_eval_accumulate.  The host evaluator stays the default and is the judge of the device path
(tests/test_coco_eval_device_gpu.py): the tables have its bits.
"""
import numpy as np


def to_float(x):
    """post_process.py:87-89"""
    return float("{:.2f}".format(x))


def convert_eval_format(detections, img_id, valid_ids):
    """detections: {class index (1-based): array [n, 5] = x1, y1, x2, y2, score} -> {"images": [...], "annotations": [...]}."""
    out = {"images": [], "annotations": []}
    for cls_ind in detections:
        class_id = valid_ids[cls_ind - 1]
        for det in detections[cls_ind]:
            d = np.asarray(det, np.float64)
            bbox = [to_float(d[0]), to_float(d[1]), to_float(d[2] - d[0]), to_float(d[3] - d[1])]
            out["annotations"].append({"image_id": int(img_id), "category_id": int(class_id), "bbox": bbox, "score": to_float(d[4])})
    if out["annotations"]:
        out["images"].append({"id": int(img_id)})
    return out


def dets_to_coco(dets, count, image_ids, valid_ids):
    """dets [B,max_det,6] (x1,y1,x2,y2,score,label 0-based), count [B] -> list of COCO result records."""
    dets, count = np.asarray(dets, np.float64), np.asarray(count)
    res = []
    for b, img_id in enumerate(image_ids):
        per_class = {}
        for d in dets[b, :int(count[b])]:
            per_class.setdefault(int(d[5]) + 1, []).append(d[:5])
        res += convert_eval_format(per_class, img_id, valid_ids)["annotations"]
    return res


def _iou_xywh(dt, gt, iscrowd):
    """[D,4] x [G,4] xywh -> [D,G]; crowd columns use intersection / detection area (pycocotools maskApi.iou semantics)."""
    if len(dt) == 0 or len(gt) == 0:
        return np.zeros((len(dt), len(gt)))
    dx1, dy1, dx2, dy2 = dt[:, 0:1], dt[:, 1:2], dt[:, 0:1] + dt[:, 2:3], dt[:, 1:2] + dt[:, 3:4]
    gx1, gy1, gx2, gy2 = gt[None, :, 0], gt[None, :, 1], gt[None, :, 0] + gt[None, :, 2], gt[None, :, 1] + gt[None, :, 3]
    iw = np.clip(np.minimum(dx2, gx2) - np.maximum(dx1, gx1), 0, None)
    ih = np.clip(np.minimum(dy2, gy2) - np.maximum(dy1, gy1), 0, None)
    inter = iw * ih
    da = (dt[:, 2] * dt[:, 3])[:, None]
    ga = (gt[:, 2] * gt[:, 3])[None, :]
    union = np.where(np.asarray(iscrowd, bool)[None, :], da, da + ga - inter)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(union > 0, inter / union, 0.0)


class COCOBboxEval:
    IOU_THRS = np.linspace(0.5, 0.95, 10)
    REC_THRS = np.linspace(0.0, 1.0, 101)
    AREA_RNG = {"all": (0, 1e10), "small": (0, 32 ** 2), "medium": (32 ** 2, 96 ** 2), "large": (96 ** 2, 1e10)}
    MAX_DETS = (1, 10, 100)

    def __init__(self, gt_annotations, dt_results, image_ids=None, category_ids=None):
        """gt_annotations: COCO "annotations" records (image_id, category_id, bbox xywh, [area], [iscrowd], [ignore]);
        dt_results: COCO result records (image_id, category_id, bbox xywh, score)."""
        self.gts, self.dts = {}, {}
        for g in gt_annotations:
            g = dict(g)
            g.setdefault("area", g["bbox"][2] * g["bbox"][3])
            g.setdefault("iscrowd", 0)
            g["_ignore"] = bool(g.get("ignore", 0)) or bool(g["iscrowd"])
            self.gts.setdefault((g["image_id"], g["category_id"]), []).append(g)
        for d in dt_results:
            d = dict(d)
            d.setdefault("area", d["bbox"][2] * d["bbox"][3])
            self.dts.setdefault((d["image_id"], d["category_id"]), []).append(d)
        keys = list(self.gts) + list(self.dts)
        self.img_ids = sorted(set(image_ids if image_ids is not None else [k[0] for k in keys]))
        self.cat_ids = sorted(set(category_ids if category_ids is not None else [k[1] for k in keys]))
        self.precision = self.recall = None

    def _evaluate_img(self, img, cat, rng, max_det):
        gts = self.gts.get((img, cat), [])
        dts = self.dts.get((img, cat), [])
        if not gts and not dts:
            return None
        g_ig = np.array([g["_ignore"] or g["area"] < rng[0] or g["area"] > rng[1] for g in gts], bool)
        g_order = np.argsort(g_ig, kind="mergesort")          # not-ignored ground truth first
        gts = [gts[i] for i in g_order]
        g_ig = g_ig[g_order]
        d_order = np.argsort([-d["score"] for d in dts], kind="mergesort")[:max_det]
        dts = [dts[i] for i in d_order]
        crowd = np.array([g["iscrowd"] for g in gts], bool)
        ious = _iou_xywh(np.array([d["bbox"] for d in dts], float).reshape(-1, 4), np.array([g["bbox"] for g in gts], float).reshape(-1, 4),
                         crowd)
        T, D, G = len(self.IOU_THRS), len(dts), len(gts)
        gtm = -np.ones((T, G), int)
        dtm = -np.ones((T, D), int)
        dt_ig = np.zeros((T, D), bool)
        for ti, t in enumerate(self.IOU_THRS):
            for di in range(D):
                iou, m = min(t, 1 - 1e-10), -1
                for gi in range(G):
                    if gtm[ti, gi] >= 0 and not crowd[gi]:
                        continue                                  # already matched (crowd may match again)
                    if m > -1 and not g_ig[m] and g_ig[gi]:
                        break                                     # a real match was found; only ignored ground truth is left
                    if ious[di, gi] < iou:
                        continue
                    iou, m = ious[di, gi], gi
                if m == -1:
                    continue
                dt_ig[ti, di] = g_ig[m]
                dtm[ti, di] = m
                gtm[ti, m] = di
        d_area = np.array([d["area"] for d in dts])
        out_of_range = (d_area < rng[0]) | (d_area > rng[1])
        dt_ig = dt_ig | ((dtm < 0) & out_of_range[None, :])     # unmatched detections outside the area range are ignored
        return dict(dt_scores=np.array([d["score"] for d in dts]), dtm=dtm, dt_ig=dt_ig, n_gt=int((~g_ig).sum()))

    @classmethod
    def from_packed(cls, packed):
        """An evaluator over a PackedCoco whose detections exist only on the device (PackedCoco.add_dets): evaluate(backend="device")."""
        ev = cls.__new__(cls)
        ev.gts, ev.dts = {}, {}
        ev.img_ids, ev.cat_ids = list(packed.img_ids), list(packed.cat_ids)
        ev.precision = ev.recall = None
        ev._packed = packed
        return ev

    def _evaluate_device(self, device=None):
        """precision / recall from md_coco_eval_match and md_coco_eval_accumulate on the packed set; one host read, of the two tables."""
        import torch

        from . import det_ops
        p = getattr(self, "_packed", None)
        if p is None:
            p = _pack_eval(self, "cuda" if device is None else device, True)
        if p.dt_box is None:
            raise ValueError("COCOBboxEval: the pack holds no detections (pack_coco(dt_results=...) or PackedCoco.add_dets)")
        if list(p.img_ids) != list(self.img_ids) or list(p.cat_ids) != list(self.cat_ids):
            raise ValueError("COCOBboxEval: the pack was made for other images or categories")
        if max(self.MAX_DETS) > MAX_CELL_DETS:
            raise ValueError(f"COCOBboxEval: the device path cuts a cell at {MAX_CELL_DETS} detections, the last maxDets value")
        dev = p.device
        const = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        dtm, dt_ig, cell_ngt = det_ops.coco_eval_match(p.gt_beg, p.gt_cnt, p.dt_beg, p.dt_cnt, p.gt_box, p.gt_area, p.gt_crowd, p.gt_ignore, p.dt_box,
                                                       p.dt_area, const(self.IOU_THRS, np.float64), const(list(self.AREA_RNG.values()), np.float64))
        order, cat_off = p.category_order()
        precision, recall, _ = det_ops.coco_eval_accumulate(order, cat_off, p.dt_rank, dtm, dt_ig, cell_ngt, const(self.REC_THRS, np.float64),
                                                            const(self.MAX_DETS, np.int32))
        self.precision, self.recall = precision.cpu().numpy(), recall.cpu().numpy()
        return self

    def evaluate(self, backend="host", device=None):
        """backend "host": the numpy evaluator below, the default and the judge of the other; "device": the md_coco_eval_* operators
        (include/minddet_hip_cocoeval.h) on pack_coco's layout, on `device` (default "cuda"); the tables have the host's bits."""
        if backend == "device":
            return self._evaluate_device(device)
        if backend != "host":
            raise ValueError(f"COCOBboxEval.evaluate: backend is \"host\" or \"device\", got {backend!r}")
        if getattr(self, "_packed", None) is not None:
            raise ValueError("COCOBboxEval.evaluate: an evaluator made from a pack has no host records; use backend=\"device\"")
        T, R, K, A, M = len(self.IOU_THRS), len(self.REC_THRS), len(self.cat_ids), len(self.AREA_RNG), len(self.MAX_DETS)
        self.precision = -np.ones((T, R, K, A, M))
        self.recall = -np.ones((T, K, A, M))
        for k, cat in enumerate(self.cat_ids):
            for a, rng in enumerate(self.AREA_RNG.values()):
                for m, max_det in enumerate(self.MAX_DETS):
                    es = [e for e in (self._evaluate_img(img, cat, rng, max_det) for img in self.img_ids) if e is not None]
                    if not es:
                        continue
                    scores = np.concatenate([e["dt_scores"] for e in es])
                    order = np.argsort(-scores, kind="mergesort")
                    dtm = np.concatenate([e["dtm"] for e in es], 1)[:, order]
                    dig = np.concatenate([e["dt_ig"] for e in es], 1)[:, order]
                    n_gt = sum(e["n_gt"] for e in es)
                    if n_gt == 0:
                        continue
                    tps = np.cumsum((dtm >= 0) & ~dig, 1).astype(float)
                    fps = np.cumsum((dtm < 0) & ~dig, 1).astype(float)
                    for ti in range(T):
                        tp, fp = tps[ti], fps[ti]
                        nd = len(tp)
                        rc = tp / n_gt
                        pr = tp / (fp + tp + np.spacing(1))
                        self.recall[ti, k, a, m] = rc[-1] if nd else 0
                        for i in range(nd - 1, 0, -1):            # precision envelope
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        inds = np.searchsorted(rc, self.REC_THRS, side="left")
                        q = np.zeros(R)
                        valid = inds < nd
                        q[valid] = pr[inds[valid]]
                        self.precision[ti, :, k, a, m] = q
        return self

    def _summarize(self, ap, iou=None, area="all", max_det=100):
        a = list(self.AREA_RNG).index(area)
        m = self.MAX_DETS.index(max_det)
        s = self.precision[:, :, :, a, m] if ap else self.recall[:, :, a, m]
        if iou is not None:
            s = s[np.isclose(self.IOU_THRS, iou)]
        s = s[s > -1]
        return float(s.mean()) if s.size else -1.0

    def summarize(self):
        """The 12 numbers COCOeval.summarize() prints, in its order."""
        if self.precision is None:
            self.evaluate()
        return {
            "AP": self._summarize(True), "AP50": self._summarize(True, 0.5), "AP75": self._summarize(True, 0.75),
            "APs": self._summarize(True, area="small"), "APm": self._summarize(True, area="medium"), "APl": self._summarize(True, area="large"),
            "AR1": self._summarize(False, max_det=1), "AR10": self._summarize(False, max_det=10), "AR100": self._summarize(False),
            "ARs": self._summarize(False, area="small"), "ARm": self._summarize(False, area="medium"), "ARl": self._summarize(False, area="large"),
        }


# ----------------------------------------------------------------------------- the device path (include/minddet_hip_cocoeval.h)
MAX_CELL_DETS, MAX_CELL_GTS, MAX_IMAGE_DETS = 100, 256, 512      # MD_COCOEVAL_MAX_DETS, MD_COCOEVAL_MAX_GTS, MD_COCOEVAL_MAX_IMAGE_DETS


class PackedCoco:
    """The records of one evaluation as flat device tensors (the layout of include/minddet_hip_cocoeval.h): I images in ascending id, Kc
    categories in ascending id, cell c = i Kc + k owning the rows [beg[c], beg[c] + cnt[c]).  Ground truth is packed once; detections come
    from records (pack_coco(dt_results=...), compact rows) or from the detector's device output (add_dets, max_det rows per image)."""

    def __init__(self, img_ids, cat_ids, device):
        self.img_ids, self.cat_ids, self.device = list(img_ids), list(cat_ids), device
        self.I, self.Kc = len(self.img_ids), len(self.cat_ids)
        self.max_det = None                                  # rows per image of the padded layout add_dets writes
        self.dt_box = self.dt_area = self.dt_score = self.dt_cat = self.dt_rank = self.dt_beg = self.dt_cnt = self.dt_src = None
        self._label_to_k = {}

    def add_dets(self, dets, count, first_image, valid_ids=None):
        """Device detections of one batch, straight from the detector and with no host read: dets [B,max_det,6] f32 (x1, y1, x2, y2,
        score, label 0-based), count [B] -> the rows and cells of the images first_image .. first_image + B - 1 (positions in img_ids),
        by md_coco_eval_rows.  valid_ids[label] is the category id, as dets_to_coco takes it (None: label l is cat_ids[l])."""
        import torch

        from . import det_ops
        if dets.dim() != 3 or dets.shape[2] != 6:
            raise ValueError(f"PackedCoco.add_dets: dets are [B, max_det, 6], got {tuple(dets.shape)}")
        B, max_det = int(dets.shape[0]), int(dets.shape[1])
        if not 1 <= max_det <= MAX_IMAGE_DETS:
            raise ValueError(f"PackedCoco.add_dets: 1 to {MAX_IMAGE_DETS} rows per image, got {max_det}")
        if first_image < 0 or first_image + B > self.I:
            raise ValueError(f"PackedCoco.add_dets: images {first_image} .. {first_image + B - 1} of {self.I}")
        if self.max_det is None:
            if self.dt_box is not None:
                raise ValueError("PackedCoco.add_dets: the pack already holds detections from records")
            dev, Dt, C = self.device, self.I * max_det, self.I * self.Kc
            if Dt > det_ops.COCOEVAL_MAX_ROWS:
                raise ValueError(f"PackedCoco.add_dets: {Dt} detection rows, at most {det_ops.COCOEVAL_MAX_ROWS}")
            self.max_det = max_det
            self.dt_box = torch.zeros((Dt, 4), dtype=torch.float64, device=dev)
            self.dt_area = torch.zeros((Dt,), dtype=torch.float64, device=dev)
            self.dt_score = torch.zeros((Dt,), dtype=torch.float64, device=dev)
            self.dt_cat = torch.full((Dt,), self.Kc, dtype=torch.int32, device=dev)      # every row unused, every cell empty
            self.dt_rank = torch.zeros((Dt,), dtype=torch.int32, device=dev)
            self.dt_beg = (torch.arange(C, dtype=torch.int32, device=dev) // self.Kc) * max_det
            self.dt_cnt = torch.zeros((C,), dtype=torch.int32, device=dev)
            self.dt_src = torch.full((Dt,), -1, dtype=torch.int32, device=dev)
        elif max_det != self.max_det:
            raise ValueError(f"PackedCoco.add_dets: {max_det} rows per image, earlier batches had {self.max_det}")
        key = None if valid_ids is None else tuple(int(v) for v in valid_ids)
        if key not in self._label_to_k:
            ids = list(self.cat_ids) if key is None else list(key)
            where = {c: k for k, c in enumerate(self.cat_ids)}
            self._label_to_k[key] = torch.tensor([where.get(c, -1) for c in ids], dtype=torch.int32, device=self.device)
        det_ops.coco_eval_rows(dets.to(self.device, torch.float32), count, self._label_to_k[key], int(first_image), self.dt_box, self.dt_area,
                               self.dt_score, self.dt_cat, self.dt_rank, self.dt_beg, self.dt_cnt, self.dt_src)
        return self

    def category_order(self):
        """-> (order [Dt] i32, cat_off [Kc+1] i32) of md_coco_eval_accumulate: the detection rows category-major, within a category in
        descending score order, equal scores in row order (two stable sorts); unused rows (dt_cat == Kc) last.  Plumbing, on the device."""
        import torch
        by_score = torch.sort(-self.dt_score, stable=True).indices
        by_cat = torch.sort(self.dt_cat[by_score], stable=True).indices
        counts = torch.bincount(self.dt_cat.long(), minlength=self.Kc + 1)[:self.Kc]
        cat_off = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).to(torch.int32)
        return by_score[by_cat].to(torch.int32), cat_off


def _pack_eval(ev, device, with_dets):
    """PackedCoco of what `ev` (a COCOBboxEval) grouped: cells in (image, category) order, a cell's ground truths in record order, its
    detections by descending score (stable) and cut at MAX_CELL_DETS, exactly as _evaluate_img takes them."""
    import torch
    p = PackedCoco(ev.img_ids, ev.cat_ids, device)
    C = p.I * p.Kc
    if p.Kc < 1 or p.I < 1:
        raise ValueError("pack_coco: at least one image and one category")
    if p.Kc > 128 or C >= 1 << 24:
        raise ValueError(f"pack_coco: at most 128 categories and fewer than 2^24 (image, category) cells, got {p.Kc} and {C}")
    g_cnt, d_cnt = np.zeros(C, np.int64), np.zeros(C, np.int64)
    g_box, g_area, g_crowd, g_ign, d_box, d_area, d_score, d_cat, d_rank = ([] for _ in range(9))
    at_i, at_k = {img: i for i, img in enumerate(p.img_ids)}, {cat: k for k, cat in enumerate(p.cat_ids)}
    keys = list(ev.gts) + (list(ev.dts) if with_dets else [])
    for c in sorted({at_i[img] * p.Kc + at_k[cat] for img, cat in keys if img in at_i and cat in at_k}):      # the cells that hold a record, in order
        img, cat, k = p.img_ids[c // p.Kc], p.cat_ids[c % p.Kc], c % p.Kc
        gts = ev.gts.get((img, cat), [])
        if len(gts) > MAX_CELL_GTS:
            raise ValueError(f"pack_coco: image {img}, category {cat} has {len(gts)} ground truths, at most {MAX_CELL_GTS}")
        g_cnt[c] = len(gts)
        for g in gts:
            g_box.append(g["bbox"]); g_area.append(g["area"]); g_crowd.append(bool(g["iscrowd"])); g_ign.append(g["_ignore"])
        if with_dets:
            dts = ev.dts.get((img, cat), [])
            for rank, j in enumerate(np.argsort([-d["score"] for d in dts], kind="mergesort")[:MAX_CELL_DETS]):
                d = dts[j]
                d_box.append(d["bbox"]); d_area.append(d["area"]); d_score.append(d["score"]); d_cat.append(k); d_rank.append(rank)
            d_cnt[c] = min(len(dts), MAX_CELL_DETS)
    g_beg, d_beg = np.cumsum(g_cnt) - g_cnt, np.cumsum(d_cnt) - d_cnt      # an empty cell begins where the next one does
    if len(g_area) > 1 << 26 or len(d_area) > 1 << 26:
        raise ValueError("pack_coco: at most 2^26 ground-truth and detection rows")
    dev_t = lambda a, dt, shape: torch.from_numpy(np.asarray(a, dt).reshape(shape)).to(device)
    p.gt_beg, p.gt_cnt = dev_t(g_beg, np.int32, (C,)), dev_t(g_cnt, np.int32, (C,))
    p.gt_box, p.gt_area = dev_t(g_box, np.float64, (-1, 4)), dev_t(g_area, np.float64, (-1,))
    p.gt_crowd, p.gt_ignore = dev_t(g_crowd, np.uint8, (-1,)), dev_t(g_ign, np.uint8, (-1,))
    if with_dets:
        p.dt_beg, p.dt_cnt = dev_t(d_beg, np.int32, (C,)), dev_t(d_cnt, np.int32, (C,))
        p.dt_box, p.dt_area, p.dt_score = dev_t(d_box, np.float64, (-1, 4)), dev_t(d_area, np.float64, (-1,)), dev_t(d_score, np.float64, (-1,))
        p.dt_cat, p.dt_rank = dev_t(d_cat, np.int32, (-1,)), dev_t(d_rank, np.int32, (-1,))
        p.dt_src = torch.arange(len(d_area), dtype=torch.int32, device=device)
    return p


def pack_coco(gt_annotations, dt_results=None, image_ids=None, category_ids=None, device="cuda"):
    """The records COCOBboxEval takes -> PackedCoco on `device`.  dt_results None: ground truth only, the detections follow through
    PackedCoco.add_dets.  A cell beyond MAX_CELL_GTS ground truths is refused (ValueError); a cell's detections are cut at MAX_CELL_DETS,
    the last maxDets value, as the host evaluator cuts them."""
    return _pack_eval(COCOBboxEval(gt_annotations, dt_results if dt_results is not None else [], image_ids, category_ids), device, dt_results is not None)
