"""The contract of the nuScenes evaluation operators (include/minddet_hip_nusceval.h): numpy statements of md_nusc_rows,
md_nusc_eval_match and md_nusc_eval_accumulate written per element (no np.interp, no np.cumsum on floats), the interval of the two
outputs that go through the device's sin / cos / atan2 (dt_quat, dt_yaw), the planted defects, and the test set that the CPU and the
GPU tests share.  Not a test module.

The test set (test_set()): I = 12 samples x Kc = 10 classes, 500 detection rows per sample, lidar coordinates and sizes on a k/8
lattice.  Samples 0 .. 8 have identity rotations and lattice translations, so global coordinates stay on the lattice and a distance of
0.5, 1, 2 or 4 is exact; samples 9 .. 11 have general poses (one with pitch and roll).  Car cells with 130, 65, 64, 63, 1 and 0 ground
truths; sample 4 with exactly 500 rows, 300 of them pedestrians; hand-made pairs in sample 5 (distances exactly at the four thresholds,
two ground truths equidistant from one detection); scores from a set of seven values (ties inside and across samples); trailer without
ground truth; construction_vehicle with ground truths and no match; ground truths without attribute, with NaN velocity, with no points
and beyond the class range; barriers and traffic cones without attributes (every attr_err NaN); barriers turned by 2 rad."""
import functools
import math

import numpy as np

from minddet_amd import nusc_eval as ne

CLASSES = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone")
I, KC, MAX_DET = 12, 10, 500
DEFECTS = ("le_threshold", "last_gt_on_tie", "lower_row_first", "one_taken_set", "period_2pi", "no_right", "nan_counted", "pairwise_sum")
U = 2.0 ** -53
TRIG_ULP = 4.0            # sin, cos and atan2 of the device: within 4 ulp of the float64 value (the bound tests/test_cp_targets_gpu.py holds them to)


# ----------------------------------------------------------------------------- the test set
@functools.lru_cache(maxsize=None)
def test_set():
    """-> dict(dets [I,500,11] f32, count [I] i32, poses [I,14] f64, gt_records, ego [I,3], dt_records): dt_records = dets_to_nusc of the rows"""
    rng = np.random.default_rng(11)
    dets, count, poses = np.zeros((I, MAX_DET, 11), np.float32), np.zeros(I, np.int32), np.zeros((I, 14))
    for i in range(I):
        poses[i] = [1, 0, 0, 0, 1.0, 0.0, 1.875, 1, 0, 0, 0, 400.0 + 16 * i, 1000.0 - 8 * i, 0.5]
    yaw_q = lambda a: [math.cos(a / 2), 0.0, 0.0, math.sin(a / 2)]
    poses[9, 0:4], poses[9, 7:11] = yaw_q(0.01), yaw_q(2.3)
    poses[10, 0:4], poses[10, 7:11] = [0.70, 0.01, -0.02, 0.71], [0.9, 0.02, 0.03, -0.43]       # pitch and roll, not normalised
    poses[11, 0:4], poses[11, 7:11] = yaw_q(-1.57), [-0.3, 0.0, 0.0, 0.95]
    poses[9:, 11:14] += [0.3, -0.7, 0.11]
    n_of = {0: [140, 10, 6, 8, 5, 20, 10, 10, 40, 20], 1: [70, 6, 4, 4, 3, 10, 6, 6, 30, 10], 2: [64, 5, 3, 3, 2, 8, 4, 4, 20, 8],
            3: [60, 5, 3, 3, 2, 8, 4, 4, 20, 8], 4: [80, 20, 10, 10, 10, 30, 10, 10, 300, 20]}
    scores = np.array([0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875], np.float32)
    for i in range(I):
        per = n_of.get(i, [12, 4, 3, 3, 2, 6, 4, 4, 10, 6])
        r = 0
        for k, n in enumerate(per):
            span = 140 if k in (5, 9) else 300 if k == 6 else 220                   # barriers and cones closer in (range 30), motorcycles beyond theirs (40)
            for _ in range(n):
                xy = rng.integers(-span, span + 1, 2) / 8
                size = rng.integers(4, 40, 3) / 8
                vel = rng.integers(-24, 25, 2) / 8 if rng.random() < 0.5 else rng.integers(-1, 2, 2) / 8
                dets[i, r] = [xy[0], xy[1], rng.integers(-8, 9) / 8, *size, *vel, rng.uniform(-3.2, 3.2), rng.choice(scores), k]
                r += 1
        count[i] = r
    assert count[4] == MAX_DET and count.max() == MAX_DET
    # the hand-made rows of sample 5 (identity rotations): appended behind the generated ones
    hand = [(6, 10.0, 10.0), (7, -5.0, -5.0), (7, -5.0, 5.0), (7, 5.0, -5.0), (7, 5.0, 5.0), (2, -20.0, -20.0)]
    r0 = int(count[5])
    for j, (k, x, y) in enumerate(hand):
        dets[5, r0 + j] = [x, y, 0.0, 1.0, 2.0, 1.5, 0.5, 0.0, 0.25, 0.5, k]
    count[5] += len(hand)
    dt_records = ne.dets_to_nusc(dets, count, poses, CLASSES)
    at, glob = 0, []
    for i in range(I):
        glob.append(dt_records[at:at + count[i]])
        at += count[i]
    offsets = [(0.0, 0.0), (0.125, 0.0), (0.5, 0.0), (0.0, 1.0), (2.0, 0.0), (0.0, 4.0), (0.375, 0.25), (3.0, 0.5), (0.0, -0.25), (1.5, 1.5)]
    gts = []

    def add(i, k, xy, size, yaw, vel, attr, num_pts=5):
        gts.append({"sample_token": i, "translation": [float(xy[0]), float(xy[1]), 1.0], "size": [float(s) for s in size],
                    "rotation": [math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)], "velocity": [float(vel[0]), float(vel[1])],
                    "detection_name": CLASSES[k], "attribute_name": attr, "num_pts": num_pts})

    want_car = {0: 130, 1: 65, 2: 64, 3: 63, 6: 1, 7: 0}
    for i in range(I):
        made = np.zeros(KC, int)
        for j, rec in enumerate(glob[i][:count[i] - (len(hand) if i == 5 else 0)]):
            k = CLASSES.index(rec["detection_name"])
            if k in (2, 4) or j % 3 == 2 or (k == 0 and i in want_car and made[0] >= want_car[i]):
                continue                                                         # no ground truth near construction vehicles, none for trailers
            off = offsets[j % len(offsets)]
            xy = np.round(np.array(rec["translation"][:2]) * 8) / 8 + off
            yaw = ne.quat_yaw(rec["rotation"]) + (2.0 if k == 5 else 0.25 * (j % 5))
            vel = [np.nan, np.nan] if j % 7 == 3 else [rec["velocity"][0] + 0.125 * (j % 4), rec["velocity"][1] - 0.25]
            attr = "" if k in (5, 9) or j % 5 == 1 else (rec["attribute_name"] if j % 2 else ne.DEFAULT_ATTR[CLASSES[k]])
            add(i, k, xy, np.array(rec["size"]) + 0.125 * (j % 3), yaw, vel, attr, 0 if j % 11 == 5 else 5)
            made[k] += j % 11 != 5                                               # a ground truth without points is dropped by the filter
        ego = poses[i, 11:13]
        near, first = len(gts), next((j for j, g in enumerate(gts) if g["sample_token"] == i), len(gts))
        while i in want_car and made[0] < want_car[i]:                           # fill the car cell to its count with lattice positions in range
            add(i, 0, ego + rng.integers(-200, 201, 2) / 8, rng.integers(8, 40, 3) / 8, 0.5, [0.0, 0.0], "vehicle.parked")
            made[0] += 1
        gts[first:] = gts[near:] + gts[first:near]                               # the fillers first: the cell's last chunk of 64 holds ground truths near detections
        add(i, 2, ego + [20.0, 20.0], [2.0, 6.0, 3.0], 0.0, [0.0, 0.0], "vehicle.parked")      # a construction vehicle far from every detection of its class
        add(i, 8, ego + [60.0, 0.0], [0.5, 0.5, 1.75], 0.0, [0.0, 0.0], "pedestrian.moving")    # beyond the pedestrian range
    e5 = poses[5, 11:13] + [1.0, 0.0]                                            # lidar (x, y) -> global, sample 5
    add(5, 6, e5 + [10.25, 10.0], [1.0, 2.0, 1.5], 0.0, [0.5, 0.0], "cycle.with_rider")
    add(5, 6, e5 + [9.75, 10.0], [1.0, 2.0, 1.5], 0.0, [0.5, 0.0], "cycle.with_rider")
    for (x, y), (ox, oy) in zip(((-5, -5), (-5, 5), (5, -5), (5, 5)), ((0.5, 0), (0, 1), (2, 0), (0, 4))):
        add(5, 7, e5 + [x + ox, y + oy], [1.0, 2.0, 1.5], 0.0, [0.5, 0.0], "cycle.without_rider")
    return dict(dets=dets, count=count, poses=poses, gt_records=gts, ego=poses[:, 11:14].copy(), dt_records=dt_records)


# ----------------------------------------------------------------------------- md_nusc_rows, per row
def _qmul(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]


def _matrix(q):
    w, x, y, z = (float(v) for v in q)
    n = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def _rot(m, v):
    return [(m[i][0] * v[0] + m[i][1] * v[1]) + m[i][2] * v[2] for i in range(3)]


def _spacing(v):
    return float(np.spacing(abs(np.float64(v))))


def _qmul_bound(a, b, db):
    """|device - host| of a b per component: b known to db per component, plus the roundings of both evaluations (4 products and 3 sums
    per component: gamma_4 of the sum of the magnitudes, on either side)"""
    a, b = [abs(float(v)) for v in a], [abs(float(v)) for v in b]
    idx = ((0, 1, 2, 3), (1, 0, 3, 2), (2, 3, 0, 1), (3, 2, 1, 0))                # component c: the b index that a[j] meets
    out = []
    for c in range(4):
        prop = sum(a[j] * db[idx[c][j]] for j in range(4))
        mag = sum(a[j] * (b[idx[c][j]] + db[idx[c][j]]) for j in range(4))
        out.append(prop + 2 * (4 * U) * 1.001 * mag)
    return out


def rows_sample(dets, count, pose, label_to_k, class_range, attr_moving, attr_still, Kc):
    """md_nusc_rows for one sample -> dict of the sample's block (max_det rows, Kc cells, beg relative to the block) plus quat_bound
    [max_det, 4] and yaw_bound [max_det]: the interval of dt_quat and dt_yaw around this evaluation."""
    max_det = len(dets)
    n = min(max(int(count), 0), max_det)
    pose = [float(v) for v in pose]
    q_cs, t_cs, q_ego, t_ego = pose[0:4], pose[4:7], pose[7:11], pose[11:14]
    m_cs, m_ego = _matrix(q_cs), _matrix(q_ego)
    keep = []
    for r in range(n):
        row = dets[r]
        yf = np.float32(-row[8]) - np.float32(np.pi / 2)
        h = float(yf) / 2
        q = [math.cos(h), 0.0, 0.0, math.sin(h)]
        dq = [TRIG_ULP * _spacing(q[0]), 0.0, 0.0, TRIG_ULP * _spacing(q[3])]
        c, v = [float(row[0]), float(row[1]), float(row[2])], [float(row[6]), float(row[7]), 0.0]
        c = [a + b for a, b in zip(_rot(m_cs, c), t_cs)]
        dq, q, v = _qmul_bound(q_cs, q, dq), _qmul(q_cs, q), _rot(m_cs, v)
        c = [a + b for a, b in zip(_rot(m_ego, c), t_ego)]
        dq, q, v = _qmul_bound(q_ego, q, dq), _qmul(q_ego, q), _rot(m_ego, v)
        m = _matrix(q)
        yaw = math.atan2(m[1][0], m[0][0])
        # the yaw interval: dq through the normalisation and the two matrix entries (first order, 1 % for the rest), then atan2
        nq = math.sqrt(sum(t * t for t in q))
        qa = [abs(t) / nq for t in q]
        dn = sum(qa[j] * dq[j] for j in range(4)) / nq
        dqn = [dq[j] / nq + qa[j] * dn + 4 * U for j in range(4)]
        d00 = 4 * (qa[2] * dqn[2] + qa[3] * dqn[3]) + 16 * U
        d10 = 2 * (qa[1] * dqn[2] + qa[2] * dqn[1] + qa[0] * dqn[3] + qa[3] * dqn[0]) + 16 * U
        den = m[0][0] ** 2 + m[1][0] ** 2
        dyaw = 1.01 * (abs(m[0][0]) * d10 + abs(m[1][0]) * d00) / den + TRIG_ULP * _spacing(yaw) if den > 0 else math.inf
        lab, sc = float(row[10]), float(row[9])
        if not (lab > -1.0 and lab < len(label_to_k)) or sc != sc:
            continue
        k = int(label_to_k[int(lab)])
        if not 0 <= k < Kc:
            continue
        ex, ey = c[0] - t_ego[0], c[1] - t_ego[1]
        if not math.sqrt(ex * ex + ey * ey) < class_range[k]:
            continue
        attr = attr_moving[k] if math.sqrt(v[0] * v[0] + v[1] * v[1]) > 0.2 else attr_still[k]
        keep.append(dict(k=k, s=sc, r=r, c=c, size=[float(t) for t in row[3:6]], q=q, v=v[:2], yaw=yaw, attr=int(attr), dq=dq, dyaw=dyaw))
    out = dict(xyz=np.zeros((max_det, 3)), size=np.zeros((max_det, 3)), quat=np.zeros((max_det, 4)), vel=np.zeros((max_det, 2)), yaw=np.zeros(max_det),
               score=np.zeros(max_det), cat=np.full(max_det, Kc, np.int32), attr=np.zeros(max_det, np.int32), rank=np.zeros(max_det, np.int32),
               src=np.full(max_det, -1, np.int32), cnt=np.zeros(Kc, np.int32), quat_bound=np.zeros((max_det, 4)), yaw_bound=np.zeros(max_det))
    for e in keep:
        out["cnt"][e["k"]] += 1
    out["beg"] = (np.cumsum(out["cnt"]) - out["cnt"]).astype(np.int32)
    for e in keep:
        rank = sum(1 for o in keep if o["k"] == e["k"] and (o["s"] > e["s"] or (o["s"] == e["s"] and o["r"] > e["r"])))
        at = out["beg"][e["k"]] + rank
        out["xyz"][at], out["size"][at], out["quat"][at], out["vel"][at], out["yaw"][at], out["score"][at] = e["c"], e["size"], e["q"], e["v"], e["yaw"], e["s"]
        out["cat"][at], out["attr"][at], out["rank"][at], out["src"][at] = e["k"], e["attr"], rank, e["r"]
        out["quat_bound"][at], out["yaw_bound"][at] = e["dq"], e["dyaw"]
    return out


# ----------------------------------------------------------------------------- md_nusc_eval_match and md_nusc_eval_accumulate, per element
def pymod(a, b):
    m = math.fmod(a, b)
    if m != 0.0:
        if (b < 0) != (m < 0):
            m += b
    else:
        m = math.copysign(0.0, b)
    return m


def interp1(x, xp, fp, right=None):
    """np.interp for one x, as include/minddet_hip_nusceval.h states it"""
    n = len(xp)
    if x != x:
        return x
    lo, hi = 0, n
    while lo < hi:
        mid = (lo + hi) >> 1
        if xp[mid] <= x:
            lo = mid + 1
        else:
            hi = mid
    j = lo - 1
    if j < 0:
        return fp[0]
    if j == n - 1:
        return right if (right is not None and x > xp[j]) else fp[j]
    if xp[j] == x:
        return fp[j]
    slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])
    v = slope * (x - xp[j]) + fp[j]
    if v != v:
        v = slope * (x - xp[j + 1]) + fp[j + 1]
        if v != v and fp[j] == fp[j + 1]:
            v = fp[j]
    return v


def _tree_sums(vals):
    """the defect "pairwise_sum": inclusive prefix sums by a doubling scan"""
    s = list(vals)
    d = 1
    while d < len(s):
        s = [s[i] + s[i - d] if i >= d else s[i] for i in range(len(s))]
        d *= 2
    return s


def tables(z, Kc, dist_ths, period, rec_thr, tp_index, defect=None):
    """The three tables and every named intermediate from packed arrays z (NuscDetectionEval.z or PackedNusc.numpy())."""
    D, R, Dt, Gt = len(dist_ths), len(rec_thr), len(z["dt_score"]), len(z["gt_yaw"])
    C = len(z["gt_beg"])
    gidx = z["dt_gidx"] if "dt_gidx" in z else z["dt_sample"].astype(np.int64) * (1 << 20) + z["dt_src"]
    tie = 1 if defect == "lower_row_first" else -1
    used = [r for r in range(Dt) if z["dt_cat"][r] < Kc]
    order = sorted(used, key=lambda r: (z["dt_cat"][r], -z["dt_score"][r], tie * gidx[r]))
    cat_off = [0] + np.cumsum(np.bincount(z["dt_cat"][used], minlength=Kc)[:Kc]).tolist()
    t = dict(dtm=-np.ones((D, Dt), np.int32), err=np.zeros((Dt, 5)), cell_ngt=np.minimum(z["gt_cnt"], 1024).astype(np.int32),
             tp_scan=np.zeros((D, Dt), np.int32), m_conf=np.zeros(Dt), m_cum=np.zeros((5, Dt)), precision=np.zeros((Kc, D, R)),
             confidence=np.zeros((Kc, D, R)), tp_err=np.ones((Kc, 5, R)), n_gt=np.zeros(Kc, np.int32), n_match=np.zeros((Kc, D), np.int32),
             order=np.array(order + [r for r in range(Dt) if z["dt_cat"][r] >= Kc], np.int32), cat_off=np.array(cat_off, np.int32))
    taken = np.zeros((D, Gt), bool)
    for r in order:                                          # the matching: a cell's rows come in the order of the list
        k = int(z["dt_cat"][r])
        c = int(z["dt_sample"][r]) * Kc + k
        g0, g1 = int(z["gt_beg"][c]), int(z["gt_beg"][c]) + int(t["cell_ngt"][c])
        dist = []
        for g in range(g0, g1):
            dx, dy = z["dt_xyz"][r, 0] - z["gt_xy"][g, 0], z["dt_xyz"][r, 1] - z["gt_xy"][g, 1]
            dist.append(math.sqrt(dx * dx + dy * dy))
        for d in range(D):
            tk = taken[0] if defect == "one_taken_set" else taken[d]
            best, hit = math.inf, -1
            for g in range(g0, g1):
                v = dist[g - g0]
                if not tk[g] and (v < best or (defect == "last_gt_on_tie" and v <= best and v < math.inf)):
                    best, hit = v, g
            ok = hit >= 0 and (best <= dist_ths[d] if defect == "le_threshold" else best < dist_ths[d])
            if not ok:
                continue
            tk[hit] = True
            t["dtm"][d, r] = hit
            if d != tp_index:
                continue
            sa, sr = z["gt_size"][hit], z["dt_size"][r]
            mn = [sa[i] if sa[i] < sr[i] else sr[i] for i in range(3)]
            va, vr, inter = (sa[0] * sa[1]) * sa[2], (sr[0] * sr[1]) * sr[2], (mn[0] * mn[1]) * mn[2]
            per = 2 * math.pi if defect == "period_2pi" else float(period[k])
            df = pymod((float(z["gt_yaw"][hit]) - float(z["dt_yaw"][r])) + per / 2, per) - per / 2
            if df > math.pi:
                df = df - 2 * math.pi
            dvx, dvy = z["gt_vel"][hit, 0] - z["dt_vel"][r, 0], z["gt_vel"][hit, 1] - z["dt_vel"][r, 1]
            ga = int(z["gt_attr"][hit])
            t["err"][r] = [best, 1 - inter / ((va + vr) - inter), abs(df), math.sqrt(dvx * dvx + dvy * dvy) if dvx == dvx and dvy == dvy else math.nan,
                           math.nan if ga < 0 else 1 - float(ga == int(z["dt_attr"][r]))]
    for k in range(Kc):
        beg, end = cat_off[k], cat_off[k + 1]
        rows = order[beg:end]
        n = end - beg
        ngt = int(sum(int(t["cell_ngt"][i * Kc + k]) for i in range(C // Kc)))
        t["n_gt"][k] = ngt
        for d in range(D):
            tp = 0
            for j, r in enumerate(rows):
                tp += int(t["dtm"][d, r] >= 0)
                t["tp_scan"][d, beg + j] = tp
            t["n_match"][k, d] = tp
            none = ngt <= 0 or tp == 0
            scan = t["tp_scan"][d, beg:end]
            if not none:
                rec = [float(scan[j]) / float(ngt) for j in range(n)]
                prec = [float(scan[j]) / (float(j + 1 - scan[j]) + float(scan[j])) for j in range(n)]
                conf = [float(z["dt_score"][r]) for r in rows]
                right = None if defect == "no_right" else 0.0
                for i in range(R):
                    t["precision"][k, d, i] = interp1(float(rec_thr[i]), rec, prec, right)
                    t["confidence"][k, d, i] = interp1(float(rec_thr[i]), rec, conf, right)
            if d != tp_index or none:
                continue
            hit = [r for r in rows if t["dtm"][d, r] >= 0]
            nm = len(hit)
            mconf = [float(z["dt_score"][r]) for r in hit]
            t["m_conf"][beg:beg + nm] = mconf
            for m in range(5):
                vals = [float(t["err"][r, m]) for r in hit]
                if all(v != v for v in vals):
                    cm = [1.0] * nm
                else:
                    zeroed = [0.0 if v != v else v for v in vals]
                    if defect == "pairwise_sum":
                        sums = _tree_sums(zeroed)
                    else:
                        sums, s = [], 0.0
                        for v in zeroed:
                            s += v
                            sums.append(s)
                    cm, cnt = [], 0
                    for j, v in enumerate(vals):
                        cnt += 1 if (defect == "nan_counted" or v == v) else 0
                        cm.append(sums[j] / float(cnt) if cnt > 0 else 0.0)
                t["m_cum"][m, beg:beg + nm] = cm
                xp, fp = mconf[::-1], cm[::-1]
                for i in range(R):
                    t["tp_err"][k, m, i] = interp1(float(t["confidence"][k, d, i]), xp, fp)
    return t
