"""nuScenes detection evaluation (the `detection_cvpr_2019` protocol) without the devkit: from CenterPoint's rows to mAP and NDS.

What it restates, host Python in the reference:
* `dets_to_nusc`: `_second_det_to_nusc_box` and `_lidar_nusc_box_to_global` (centerpoint/det3d_ms/datasets/nuscenes/nusc_common.py:160-201)
  and the attribute rule and record format of nuscenes.py:252-293, from the fixed-shape device output `dets [B, max_det, 11]`
  (x, y, z, dx, dy, dz, vx, vy, rot, score, label) + `count [B]` of md_cp_pack.
* `NuscDetectionEval`: the devkit's `DetectionEval` the reference calls at nusc_common.py:659-674: the class-range filter, the greedy
  centre-distance matching per (class, distance threshold), the 101-point precision / confidence curves, the running-mean true-positive
  error curves, AP, the five TP metrics, mAP and NDS.
The devkit and pyquaternion are not installable here, so the protocol is written out below and this evaluator is checked against
hand-computed answers and recorded vectors of the reference's own formatting (tests/test_nusc_eval_cpu.py); parity with the devkit's own
bits is unpinned.  The bike-rack filter of the devkit (predictions and ground truths of bicycles and motorcycles inside a bike rack are
removed) needs the map annotations of the data set and is out of scope.

Quaternions are (w, x, y, z).  The conventions, this project's choice, stated once:
* product (Hamilton), evaluated left to right on the quaternions as given (not normalised):
    (a b).w = aw bw - ax bx - ay by - az bz      (a b).x = aw bx + ax bw + ay bz - az by
    (a b).y = aw by - ax bz + ay bw + az bx      (a b).z = aw bz + ax by - ay bx + az bw
* rotation matrix of q: n = sqrt(((w w + x x) + y y) + z z), every component divided by n, then
    [[1 - 2 (y y + z z), 2 (x y - w z),     2 (x z + w y)],
     [2 (x y + w z),     1 - 2 (x x + z z), 2 (y z - w x)],
     [2 (x z - w y),     2 (y z + w x),     1 - 2 (x x + y y)]]
  and R v = ((r0 vx + r1 vy) + r2 vz) per row.
* a box: yaw' = float32(-rot) - float32(pi / 2) in float32 (the reference evaluates it on the float32 array), q_box = (cos(yaw' / 2), 0, 0,
  sin(yaw' / 2)) in float64; centre, velocity (vx, vy, 0) and size widened to float64; then, as _lidar_nusc_box_to_global:
  rotate by cs_rotation, translate by cs_translation, rotate by ego_rotation, translate by ego_translation, where "rotate by r" is
  centre = R(r) centre, orientation = r orientation, velocity = R(r) velocity.
* yaw of an orientation q: atan2(r10, r00) of R(q), the direction of the rotated x axis.  A record may carry "yaw": the evaluator then takes
  it as it lies (rows_to_results writes the device's value there, so that both backends judge the same number).

Host numpy, float64.  The device path (the end of this file; include/minddet_hip_nusceval.h): pack_nusc lays the filtered records out as flat
tensors per (sample, class) cell, PackedNusc.add_dets takes the detector's (dets, count) straight from the device (md_nusc_rows),
NuscDetectionEval.evaluate(backend="device") / from_packed fill the tables from md_nusc_eval_match and md_nusc_eval_accumulate;
summarize() stays on the host in both.  The host evaluator is the default and the judge of the device path.
"""
import math

import numpy as np

ATTRIBUTES = ("cycle.with_rider", "cycle.without_rider", "pedestrian.moving", "pedestrian.sitting_lying_down", "pedestrian.standing",
              "vehicle.moving", "vehicle.parked", "vehicle.stopped")          # the order of cls_attr_dist's keys (nusc_common.py:46); code -1: none
# the most frequent attribute of a class in cls_attr_dist, the first one on equal counts (barrier and traffic_cone: all counts are 0)
DEFAULT_ATTR = {"barrier": "cycle.with_rider", "bicycle": "cycle.without_rider", "bus": "vehicle.moving", "car": "vehicle.parked",
                "construction_vehicle": "vehicle.parked", "motorcycle": "cycle.without_rider", "pedestrian": "pedestrian.moving",
                "traffic_cone": "cycle.with_rider", "trailer": "vehicle.parked", "truck": "vehicle.parked"}
DETECTION_CVPR_2019 = dict(
    class_range={"car": 50, "truck": 50, "bus": 50, "trailer": 50, "construction_vehicle": 50, "pedestrian": 40, "motorcycle": 40, "bicycle": 40,
                 "traffic_cone": 30, "barrier": 30},
    dist_ths=(0.5, 1.0, 2.0, 4.0), dist_th_tp=2.0, min_recall=0.1, min_precision=0.1, max_boxes_per_sample=500, mean_ap_weight=5)
TP_METRICS = ("trans_err", "scale_err", "orient_err", "vel_err", "attr_err")
SPEED_MOVING = 0.2
POSE_KEYS = ("cs_rotation", "cs_translation", "ego_rotation", "ego_translation")


def attr_code(name):
    return ATTRIBUTES.index(name) if name else -1


def attr_tables(class_names):
    """-> (attr_moving [Kc], attr_still [Kc]) attribute codes: the rule of nuscenes.py:258-291 per class for v > 0.2 and otherwise"""
    moving, still = [], []
    for n in class_names:
        default = DEFAULT_ATTR[n]
        moving.append(attr_code("vehicle.moving" if n in ("car", "construction_vehicle", "bus", "truck", "trailer") else
                                "cycle.with_rider" if n in ("bicycle", "motorcycle") else default))
        still.append(attr_code("pedestrian.standing" if n == "pedestrian" else "vehicle.stopped" if n == "bus" else default))
    return np.array(moving, np.int32), np.array(still, np.int32)


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], np.float64)


def quat_matrix(q):
    w, x, y, z = (np.float64(v) for v in q)
    n = np.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], np.float64)


def mat_vec(r, v):
    return np.array([(r[i][0] * v[0] + r[i][1] * v[1]) + r[i][2] * v[2] for i in range(3)], np.float64)


def quat_yaw(q):
    r = quat_matrix(q)
    return float(np.arctan2(r[1][0], r[0][0]))


def pose_array(poses):
    """poses: [B, 14] numbers, or B dicts of cs_rotation, cs_translation, ego_rotation, ego_translation -> [B, 14] f64"""
    if len(poses) and isinstance(poses[0], dict):
        poses = [np.concatenate([np.asarray(p[k], np.float64) for k in POSE_KEYS]) for p in poses]
    return np.asarray(poses, np.float64).reshape(-1, 14)


def box_to_global(row, pose):
    """one float32 row (x, y, z, dx, dy, dz, vx, vy, rot) under one pose [14] -> centre [3], size [3], orientation [4], velocity [3], f64"""
    row = np.asarray(row, np.float32)
    yaw = np.float32(-row[8]) - np.float32(np.pi / 2)
    half = np.float64(yaw) / 2
    q = np.array([np.cos(half), 0.0, 0.0, np.sin(half)], np.float64)
    c, v = row[:3].astype(np.float64), np.array([row[6], row[7], 0.0], np.float64)
    for rot, tr in ((pose[0:4], pose[4:7]), (pose[7:11], pose[11:14])):
        r = quat_matrix(rot)
        c, q, v = mat_vec(r, c) + tr, quat_mul(rot, q), mat_vec(r, v)
    return c, row[3:6].astype(np.float64), q, v


def dets_to_nusc(dets, count, poses, class_names, tokens=None):
    """dets [B, max_det, 11] f32 (the 9 box values, score, label), count [B], poses (pose_array), class_names[label] -> the records of
    the nuScenes submission format, sample by sample in row order (sample_token: tokens[b], default b)."""
    dets, count, poses = np.asarray(dets, np.float32), np.asarray(count), pose_array(poses)
    moving, still = attr_tables(class_names)
    res = []
    for b in range(dets.shape[0]):
        for d in dets[b, :int(count[b])]:
            c, size, q, v = box_to_global(d[:9], poses[b])
            k = int(d[10])
            attr = (moving if np.sqrt(v[0] ** 2 + v[1] ** 2) > SPEED_MOVING else still)[k]
            res.append({"sample_token": b if tokens is None else tokens[b], "translation": c.tolist(), "size": size.tolist(), "rotation": q.tolist(),
                        "velocity": v[:2].tolist(), "detection_name": class_names[k], "detection_score": float(d[9]),
                        "attribute_name": ATTRIBUTES[attr]})
    return res


# ----------------------------------------------------------------------------- the evaluator
def _group(records, tokens, ego, class_names, is_gt, cfg):
    """records -> the kept boxes as flat arrays in packed order: cell-major (sample, class), ground truths in record order, detections
    in walking order (descending (score, global index)); the filter of the devkit's load_prediction / filter_eval_boxes"""
    at = {t: i for i, t in enumerate(tokens)}
    Kc, I = len(class_names), len(tokens)
    per_sample = np.zeros(I, np.int64)
    rows = []
    by_sample = sorted(range(len(records)), key=lambda j: at[records[j]["sample_token"]])      # stable: the global index
    for gidx, j in enumerate(by_sample):
        r = records[j]
        i = at[r["sample_token"]]
        per_sample[i] += 1
        name = r["detection_name"]
        if name not in class_names or name not in cfg["class_range"]:
            continue
        t = np.asarray(r["translation"], np.float64)
        dx, dy = t[0] - ego[i][0], t[1] - ego[i][1]
        if not np.sqrt(dx * dx + dy * dy) < cfg["class_range"][name]:
            continue
        if is_gt and int(r.get("num_pts", 1)) == 0:
            continue
        score = float(r.get("detection_score", -1.0))
        if not is_gt and math.isnan(score):
            raise ValueError("NuscDetectionEval: a detection score is NaN")
        yaw = float(r["yaw"]) if "yaw" in r else quat_yaw(r["rotation"])
        vel = np.asarray(r.get("velocity", (np.nan, np.nan)), np.float64)[:2]
        rows.append((i, class_names.index(name), gidx, score, t, np.asarray(r["size"], np.float64), np.asarray(r["rotation"], np.float64), yaw, vel,
                     attr_code(r.get("attribute_name", ""))))
    if not is_gt and per_sample.max(initial=0) > cfg["max_boxes_per_sample"]:
        raise ValueError(f"NuscDetectionEval: a sample has {per_sample.max()} predictions, at most {cfg['max_boxes_per_sample']}")
    rows.sort(key=(lambda r: (r[0], r[1], r[2])) if is_gt else (lambda r: (r[0], r[1], -r[3], -r[2])))
    n = len(rows)
    col = lambda j, dt, shape: np.array([r[j] for r in rows], dt).reshape(shape)
    cells = col(0, np.int64, (n,)) * Kc + col(1, np.int64, (n,))
    cnt = np.bincount(cells, minlength=I * Kc).astype(np.int32)
    beg = (np.cumsum(cnt) - cnt).astype(np.int32)
    p = "gt_" if is_gt else "dt_"
    z = {p + "beg": beg, p + "cnt": cnt, p + "sample": col(0, np.int32, (n,)), p + "cat": col(1, np.int32, (n,)), p + "gidx": col(2, np.int64, (n,)),
         p + "xyz": col(4, np.float64, (n, 3)), p + "size": col(5, np.float64, (n, 3)), p + "quat": col(6, np.float64, (n, 4)),
         p + "yaw": col(7, np.float64, (n,)), p + "vel": col(8, np.float64, (n, 2)), p + "attr": col(9, np.int32, (n,))}
    if is_gt:
        z["gt_xy"] = np.ascontiguousarray(z["gt_xyz"][:, :2])
    else:
        z["dt_score"] = col(3, np.float64, (n,))
        z["dt_rank"] = (np.arange(n) - beg[cells]).astype(np.int32)
        z["dt_src"] = z["dt_gidx"].astype(np.int32)
    return z


def angle_diff(x, y, period):
    d = (x - y + period / 2) % period - period / 2
    if d > np.pi:
        d = d - 2 * np.pi
    return d


def cummean(x):
    if np.isnan(x).sum() == len(x):
        return np.ones(len(x))
    s, c = np.nancumsum(x.astype(float)), np.cumsum(~np.isnan(x))
    return np.divide(s, c, out=np.zeros_like(s), where=c != 0)


class NuscDetectionEval:
    def __init__(self, gt_records, dt_records, ego_translations, class_names, config=None):
        """gt_records: sample_token, translation, size, rotation (or yaw), velocity, detection_name, attribute_name ("" for none), num_pts;
        dt_records: the same with detection_score; ego_translations: {sample_token: (x, y, z)} in sample order, or a sequence (the
        tokens are then 0 .. I - 1); class_names: the Kc evaluated classes, k = the position."""
        self.cfg = dict(DETECTION_CVPR_2019 if config is None else config)
        self.class_names = list(class_names)
        self.tokens = list(ego_translations) if isinstance(ego_translations, dict) else list(range(len(ego_translations)))
        self.ego = np.array([ego_translations[t] for t in self.tokens], np.float64).reshape(-1, 3)
        self.z = dict(_group(gt_records, self.tokens, self.ego, self.class_names, True, self.cfg))
        if dt_records is not None:
            self.z.update(_group(dt_records, self.tokens, self.ego, self.class_names, False, self.cfg))
        self._packed = None
        self.tables = None

    @classmethod
    def from_arrays(cls, z, class_names, config=None):
        """An evaluator on packed arrays as they lie (PackedNusc.numpy(): device rows read back); rows with dt_cat == Kc are unused."""
        ev = cls.__new__(cls)
        ev.cfg, ev.class_names = dict(DETECTION_CVPR_2019 if config is None else config), list(class_names)
        ev.z, ev._packed, ev.tables = dict(z), None, None
        if "dt_gidx" not in ev.z:                             # the global index: samples in order, then source rows in order
            ev.z["dt_gidx"] = ev.z["dt_sample"].astype(np.int64) * (1 << 20) + ev.z["dt_src"]
        return ev

    @classmethod
    def from_packed(cls, packed):
        """An evaluator over a PackedNusc whose detections exist only on the device (PackedNusc.add_dets): evaluate(backend="device")."""
        ev = cls.__new__(cls)
        ev.cfg, ev.class_names = dict(packed.cfg), list(packed.class_names)
        ev.z, ev._packed, ev.tables = None, packed, None
        return ev

    def periods(self):
        return np.array([np.pi if n == "barrier" else 2 * np.pi for n in self.class_names], np.float64)

    def tp_index(self):
        return list(self.cfg["dist_ths"]).index(self.cfg["dist_th_tp"])

    def evaluate(self, backend="host", device=None):
        """Fills self.tables: precision, confidence [Kc, D, 101], tp_err [Kc, 5, 101] (at dist_th_tp), n_gt [Kc], n_match [Kc, D] and the
        intermediates in the packed layout (dtm [D, Dt], err [Dt, 5], cell_ngt, order, cat_off, tp_scan [D, Dt], m_conf [Dt],
        m_cum [5, Dt]).  backend "host": numpy, the default and the judge; "device": the md_nusc_eval_* operators, the same bits; only the
        first five tables are read back, every result stays on the device in self.device_tables."""
        if backend == "device":
            return self._evaluate_device(device)
        if backend != "host":
            raise ValueError(f"NuscDetectionEval.evaluate: backend is \"host\" or \"device\", got {backend!r}")
        if self.z is None or "dt_score" not in self.z:
            raise ValueError("NuscDetectionEval.evaluate: no host detections; use backend=\"device\" on a pack")
        z, Kc, ths, R = self.z, len(self.class_names), list(self.cfg["dist_ths"]), 101
        D, Dt, tpi, period = len(ths), len(z["dt_score"]), self.tp_index(), self.periods()
        rec_interp = np.linspace(0, 1, R)
        t = dict(precision=np.zeros((Kc, D, R)), confidence=np.zeros((Kc, D, R)), tp_err=np.ones((Kc, 5, R)), n_gt=np.zeros(Kc, np.int32),
                 n_match=np.zeros((Kc, D), np.int32), dtm=-np.ones((D, Dt), np.int32), err=np.zeros((Dt, 5)), cell_ngt=z["gt_cnt"].copy(),
                 tp_scan=np.zeros((D, Dt), np.int32), m_conf=np.zeros(Dt), m_cum=np.zeros((5, Dt)))
        order, cat_off = [], [0]
        for k in range(Kc):
            rows = np.nonzero(z["dt_cat"] == k)[0].tolist()
            walk = sorted(rows, key=lambda r: (z["dt_score"][r], z["dt_gidx"][r]))[::-1]
            base = len(order)
            order += walk
            cat_off.append(len(order))
            npos = int(z["gt_cnt"][k::Kc].sum())
            t["n_gt"][k] = npos
            for d, th in enumerate(ths):
                taken = np.zeros(len(z["gt_yaw"]), bool)
                tp, conf, md, mconf = [], [], [], []
                for r in walk:
                    c = int(z["dt_sample"][r]) * Kc + k
                    g0, g1 = int(z["gt_beg"][c]), int(z["gt_beg"][c] + z["gt_cnt"][c])
                    hit, best = -1, np.inf
                    if g1 > g0:
                        dx, dy = z["dt_xyz"][r, 0] - z["gt_xy"][g0:g1, 0], z["dt_xyz"][r, 1] - z["gt_xy"][g0:g1, 1]
                        dist = np.sqrt(dx * dx + dy * dy)
                        dist = np.where(taken[g0:g1] | ~(dist < np.inf), np.inf, dist)
                        j = int(np.argmin(dist))                      # the first minimum
                        if dist[j] < best:
                            hit, best = g0 + j, dist[j]
                    ok = hit >= 0 and best < th
                    tp.append(int(ok))
                    conf.append(z["dt_score"][r])
                    if not ok:
                        continue
                    taken[hit] = True
                    t["dtm"][d, r] = hit
                    dv = z["gt_vel"][hit] - z["dt_vel"][r]
                    sa, sr = z["gt_size"][hit], z["dt_size"][r]
                    mn = np.minimum(sa, sr)
                    va, vr, inter = (sa[0] * sa[1]) * sa[2], (sr[0] * sr[1]) * sr[2], (mn[0] * mn[1]) * mn[2]
                    ga = z["gt_attr"][hit]
                    e = [best, 1 - inter / ((va + vr) - inter), abs(angle_diff(z["gt_yaw"][hit], z["dt_yaw"][r], period[k])),
                         np.sqrt(dv[0] * dv[0] + dv[1] * dv[1]), np.nan if ga < 0 else 1 - float(ga == z["dt_attr"][r])]
                    md.append(e)
                    mconf.append(z["dt_score"][r])
                    if d == tpi:
                        t["err"][r] = e
                n = len(walk)
                tps = np.cumsum(np.array(tp, np.int64))
                t["tp_scan"][d, base:base + n] = tps
                t["n_match"][k, d] = len(md)
                if npos == 0 or not md:
                    continue                                          # the "no predictions" tables: 0, 0 and 1
                tpf = tps.astype(float)
                fpf = np.cumsum(1 - np.array(tp, np.int64)).astype(float)
                prec, rec = tpf / (fpf + tpf), tpf / float(npos)
                t["precision"][k, d] = np.interp(rec_interp, rec, prec, right=0)
                confidence = np.interp(rec_interp, rec, np.array(conf), right=0)
                t["confidence"][k, d] = confidence
                if d != tpi:
                    continue
                mconf, md = np.array(mconf), np.array(md)
                t["m_conf"][base:base + len(mconf)] = mconf
                for m in range(5):
                    cm = cummean(md[:, m])
                    t["m_cum"][m, base:base + len(cm)] = cm
                    t["tp_err"][k, m] = np.interp(confidence[::-1], mconf[::-1], cm[::-1])[::-1]
        t["order"], t["cat_off"] = np.array(order + [r for r in range(Dt) if z["dt_cat"][r] >= Kc], np.int32), np.array(cat_off, np.int32)
        self.tables = t
        return self

    def _evaluate_device(self, device=None):
        import torch

        from . import det_ops
        p = self._packed
        if p is None:
            p = self._packed = PackedNusc.from_arrays(self.z, self.tokens, self.ego, self.class_names, "cuda" if device is None else device, self.cfg)
        if p.dt_score is None:
            raise ValueError("NuscDetectionEval: the pack holds no detections (pack_nusc(dt_records=...) or PackedNusc.add_dets)")
        dev = p.device
        const = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
        tpi = self.tp_index()
        dtm, err, cell_ngt = det_ops.nusc_eval_match(p.gt_beg, p.gt_cnt, p.dt_beg, p.dt_cnt, p.gt_xy, p.gt_size, p.gt_yaw, p.gt_vel, p.gt_attr, p.dt_xyz,
                                                     p.dt_size, p.dt_yaw, p.dt_vel, p.dt_attr, const(self.cfg["dist_ths"]), const(self.periods()), tpi)
        order, cat_off = p.category_order()
        out = det_ops.nusc_eval_accumulate(order, cat_off, p.dt_score, dtm, err, cell_ngt, const(np.linspace(0, 1, 101)), tpi)
        names = ("precision", "confidence", "tp_err", "n_gt", "n_match", "tp_scan", "m_conf", "m_cum")
        self.device_tables = dict(zip(names + ("dtm", "err", "cell_ngt", "order", "cat_off"), out + (dtm, err, cell_ngt, order, cat_off)))
        self.tables = {n: self.device_tables[n].cpu().numpy() for n in names[:5]}      # the one host read: what summarize() takes
        return self

    def summarize(self):
        """-> dict: label_aps {class: {dist_th: AP}}, label_tp_errors {class: {metric: value}}, mean_dist_aps, mean_ap, tp_errors,
        tp_scores, nd_score: the fields of the devkit's DetectionMetrics.serialize() that the tables determine."""
        if self.tables is None:
            self.evaluate()
        t, cfg = self.tables, self.cfg
        first = round(100 * cfg["min_recall"]) + 1
        aps, tps = {}, {}
        for k, name in enumerate(self.class_names):
            aps[name] = {}
            for d, th in enumerate(cfg["dist_ths"]):
                prec = np.copy(t["precision"][k, d])[first:] - cfg["min_precision"]
                prec[prec < 0] = 0
                aps[name][th] = float(np.mean(prec)) / (1.0 - cfg["min_precision"])
            nz = np.nonzero(t["confidence"][k, self.tp_index()])[0]
            last = int(nz[-1]) if len(nz) else 0
            tps[name] = {}
            for m, metric in enumerate(TP_METRICS):
                if (name == "traffic_cone" and metric in ("attr_err", "vel_err", "orient_err")) or (name == "barrier" and metric in ("attr_err", "vel_err")):
                    tps[name][metric] = float("nan")
                else:
                    tps[name][metric] = 1.0 if last < first else float(np.mean(t["tp_err"][k, m, first:last + 1]))
        mean_dist_aps = {n: float(np.mean(list(v.values()))) for n, v in aps.items()}
        mean_ap = float(np.mean(list(mean_dist_aps.values())))
        tp_errors = {m: float(np.nanmean([tps[n][m] for n in self.class_names])) for m in TP_METRICS}
        tp_scores = {m: max(1.0 - v, 0.0) for m, v in tp_errors.items()}
        w = float(cfg["mean_ap_weight"])
        nd = (w * mean_ap + float(np.sum(list(tp_scores.values())))) / (w + len(tp_scores))
        return dict(label_aps=aps, label_tp_errors=tps, mean_dist_aps=mean_dist_aps, mean_ap=mean_ap, tp_errors=tp_errors, tp_scores=tp_scores, nd_score=nd)


# ----------------------------------------------------------------------------- the device path (include/minddet_hip_nusceval.h)
MAX_SAMPLE_DETS, MAX_CELL_GTS, MAX_CLASSES, MAX_THRS = 512, 1024, 16, 8      # MD_NUSCEVAL_MAX_SAMPLE_DETS, _MAX_GTS, _MAX_CLASSES, _MAX_THRS
GT_NAMES = ("gt_beg", "gt_cnt", "gt_xy", "gt_size", "gt_yaw", "gt_vel", "gt_attr")
DT_NAMES = ("dt_xyz", "dt_size", "dt_quat", "dt_vel", "dt_yaw", "dt_score", "dt_cat", "dt_attr", "dt_rank", "dt_src", "dt_beg", "dt_cnt")
_F64_NAMES = ("gt_xy", "gt_size", "gt_yaw", "gt_vel", "dt_xyz", "dt_size", "dt_quat", "dt_vel", "dt_yaw", "dt_score")


class PackedNusc:
    """The boxes of one evaluation as flat device tensors (the layout of include/minddet_hip_nusceval.h): I samples in order, Kc classes,
    cell c = i Kc + k owning the rows [beg[c], beg[c] + cnt[c]).  Ground truth is packed once (filtered); detections come from records
    (pack_nusc(dt_records=...), compact rows) or from the detector's device output (add_dets, max_det rows per sample)."""

    def __init__(self, tokens, ego, class_names, device, cfg=None):
        self.tokens, self.ego, self.class_names, self.device = list(tokens), np.asarray(ego, np.float64).reshape(-1, 3), list(class_names), device
        self.cfg = dict(DETECTION_CVPR_2019 if cfg is None else cfg)
        self.I, self.Kc = len(self.tokens), len(self.class_names)
        if self.I < 1 or not 1 <= self.Kc <= MAX_CLASSES:
            raise ValueError(f"pack_nusc: at least one sample and 1 to {MAX_CLASSES} classes, got {self.I} and {self.Kc}")
        if len(self.cfg["dist_ths"]) > MAX_THRS:
            raise ValueError(f"pack_nusc: at most {MAX_THRS} distance thresholds")
        self.max_det = None
        for n in DT_NAMES + ("dt_sample",):
            setattr(self, n, None)
        self._const = {}

    @classmethod
    def from_arrays(cls, z, tokens, ego, class_names, device, cfg=None):
        import torch
        p = cls(tokens, ego, class_names, device, cfg)
        if int(z["gt_cnt"].max(initial=0)) > MAX_CELL_GTS:
            raise ValueError(f"pack_nusc: a (sample, class) cell has {int(z['gt_cnt'].max())} ground truths, at most {MAX_CELL_GTS}")
        for n in GT_NAMES + ((DT_NAMES + ("dt_sample",)) if "dt_score" in z else ()):
            setattr(p, n, torch.from_numpy(np.ascontiguousarray(z[n], np.float64 if n in _F64_NAMES else np.int32)).to(device))
        return p

    def numpy(self):
        """every operand read back -> the dict NuscDetectionEval.from_arrays takes"""
        return {n: getattr(self, n).cpu().numpy() for n in GT_NAMES + DT_NAMES + ("dt_sample",) if getattr(self, n) is not None}

    def constants(self, class_names):
        """the device constants of add_dets for the detector's label names: label_to_k, class_range, attr_moving, attr_still"""
        import torch
        key = tuple(class_names)
        if key not in self._const:
            l2k = [self.class_names.index(n) if n in self.class_names and n in self.cfg["class_range"] else -1 for n in key]
            mv, st = attr_tables(self.class_names)
            rng = np.array([self.cfg["class_range"][n] for n in self.class_names], np.float64)
            self._const[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in (np.array(l2k, np.int32), rng, mv, st))
        return self._const[key]

    def add_dets(self, dets, count, poses, first_sample, class_names=None):
        """Device detections of one batch, straight from md_cp_pack and with no host read: dets [B, max_det, 11] f32, count [B] i32, poses
        (pose_array; a [B, 14] f64 device tensor is taken as it lies) -> the rows and cells of the samples first_sample ..
        first_sample + B - 1, by md_nusc_rows.  class_names[label]: the detector's names (default: the pack's).  max_det is at most
        max_boxes_per_sample (500): the devkit refuses a sample with more predictions, and count is not read here."""
        import torch

        from . import det_ops
        if dets.dim() != 3 or dets.shape[2] != 11:
            raise ValueError(f"PackedNusc.add_dets: dets are [B, max_det, 11], got {tuple(dets.shape)}")
        B, max_det = int(dets.shape[0]), int(dets.shape[1])
        if not 1 <= max_det <= min(MAX_SAMPLE_DETS, self.cfg["max_boxes_per_sample"]):
            raise ValueError(f"PackedNusc.add_dets: 1 to {min(MAX_SAMPLE_DETS, self.cfg['max_boxes_per_sample'])} rows per sample, got {max_det}")
        if first_sample < 0 or first_sample + B > self.I:
            raise ValueError(f"PackedNusc.add_dets: samples {first_sample} .. {first_sample + B - 1} of {self.I}")
        if self.max_det is None:
            if self.dt_score is not None:
                raise ValueError("PackedNusc.add_dets: the pack already holds detections from records")
            dev, Dt, C = self.device, self.I * max_det, self.I * self.Kc
            if Dt > det_ops.NUSCEVAL_MAX_ROWS:
                raise ValueError(f"PackedNusc.add_dets: {Dt} detection rows, at most {det_ops.NUSCEVAL_MAX_ROWS}")
            self.max_det = max_det
            f = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
            self.dt_xyz, self.dt_size, self.dt_quat, self.dt_vel, self.dt_yaw, self.dt_score = f(Dt, 3), f(Dt, 3), f(Dt, 4), f(Dt, 2), f(Dt), f(Dt)
            self.dt_cat = torch.full((Dt,), self.Kc, dtype=torch.int32, device=dev)      # every row unused, every cell empty
            self.dt_attr, self.dt_rank = (torch.zeros((Dt,), dtype=torch.int32, device=dev) for _ in range(2))
            self.dt_src = torch.full((Dt,), -1, dtype=torch.int32, device=dev)
            self.dt_beg = (torch.arange(C, dtype=torch.int32, device=dev) // self.Kc) * max_det
            self.dt_cnt = torch.zeros((C,), dtype=torch.int32, device=dev)
            self.dt_sample = torch.arange(Dt, dtype=torch.int32, device=dev) // max_det
        elif max_det != self.max_det:
            raise ValueError(f"PackedNusc.add_dets: {max_det} rows per sample, earlier batches had {self.max_det}")
        if not torch.is_tensor(poses):
            poses = torch.from_numpy(pose_array(poses))
        l2k, rng, mv, st = self.constants(self.class_names if class_names is None else class_names)
        det_ops.nusc_rows(dets.to(self.device, torch.float32), count, poses.to(self.device, torch.float64), l2k, rng, mv, st, int(first_sample),
                          *[getattr(self, n) for n in DT_NAMES])
        return self

    def category_order(self):
        """-> (order [Dt] i32, cat_off [Kc+1] i32) of md_nusc_eval_accumulate: the detection rows class-major, within a class in walking
        order across the samples: descending score, equal scores the later sample first and, inside a sample, in row order (three
        stable sorts); unused rows (dt_cat == Kc) last.  Plumbing, on the device."""
        import torch
        Dt = self.dt_cat.shape[0]
        tie = (self.I - 1 - self.dt_sample.long()) * Dt + torch.arange(Dt, device=self.dt_cat.device)
        by_tie = torch.sort(tie, stable=True).indices
        by_score = by_tie[torch.sort(-self.dt_score[by_tie], stable=True).indices]
        by_cat = torch.sort(self.dt_cat[by_score], stable=True).indices
        counts = torch.bincount(self.dt_cat.long(), minlength=self.Kc + 1)[:self.Kc]
        cat_off = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).to(torch.int32)
        return by_score[by_cat].to(torch.int32), cat_off


def pack_nusc(gt_records, ego_translations, class_names, device="cuda", dt_records=None, config=None):
    """The records NuscDetectionEval takes -> PackedNusc on `device`, filtered as the evaluator filters.  dt_records None: ground truth
    only, the detections follow through PackedNusc.add_dets.  A cell beyond MAX_CELL_GTS ground truths is refused (ValueError)."""
    ev = NuscDetectionEval(gt_records, dt_records, ego_translations, class_names, config)
    return PackedNusc.from_arrays(ev.z, ev.tokens, ev.ego, ev.class_names, device, ev.cfg)


def rows_to_results(packed):
    """The submission dict of nuscenes.py:279-302 from a pack's detection rows (one host read): {"results": {sample_token: [records]},
    "meta": {...}}, a sample's records in source-row order.  Only the rows the filter kept exist.  Each record also carries "yaw", the
    stored dt_yaw, which NuscDetectionEval takes in place of its own atan2."""
    z = packed.numpy()
    results = {t: [] for t in packed.tokens}
    rows = [r for r in range(len(z["dt_cat"])) if z["dt_cat"][r] < packed.Kc]
    for r in sorted(rows, key=lambda r: (z["dt_sample"][r], z["dt_src"][r])):
        results[packed.tokens[z["dt_sample"][r]]].append({
            "sample_token": packed.tokens[z["dt_sample"][r]], "translation": z["dt_xyz"][r].tolist(), "size": z["dt_size"][r].tolist(),
            "rotation": z["dt_quat"][r].tolist(), "velocity": z["dt_vel"][r].tolist(), "detection_name": packed.class_names[z["dt_cat"][r]],
            "detection_score": float(z["dt_score"][r]), "attribute_name": ATTRIBUTES[z["dt_attr"][r]], "yaw": float(z["dt_yaw"][r])})
    meta = {"use_camera": False, "use_lidar": True, "use_radar": False, "use_map": False, "use_external": False}
    return {"results": results, "meta": meta}
