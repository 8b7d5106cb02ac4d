"""CPU: minddet_amd/nusc_eval.py's formatting against recorded vectors of the reference's own routines
(tests/golden/nusc_rows_vectors.json, written by tests/golden/gen_nusc_rows.py from _second_det_to_nusc_box and
_lidar_nusc_box_to_global): the float32 yaw step and everything polynomial (centres, sizes, velocities) exact, the quaternions within
the interval of tests/nusc_eval_contract.py (sin and cos within 4 ulp, propagated through the two Hamilton products); the records of
dets_to_nusc and the filter of the evaluator."""
import json
import os

import numpy as np

from minddet_amd import nusc_eval as ne
from tests import nusc_eval_contract as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "nusc_rows_vectors.json")))


def test_box_to_global_equals_the_reference_routines():
    assert set(GOLD) == {"yaw", "tilt", "scaled"} and sum(len(c["boxes"]) for c in GOLD.values()) >= 40
    for name, case in GOLD.items():
        pose = np.array(case["pose"], np.float64)
        for j, box in enumerate(case["boxes"]):
            row = np.array(box, np.float32)
            assert row.astype(np.float64).tolist() == box                          # float32 inputs
            c, size, q, v = ne.box_to_global(row, pose)
            assert c.tolist() == case["center"][j] and size.tolist() == case["size"][j] and v.tolist() == case["velocity"][j], (name, j)
            h = float(np.float32(-row[8]) - np.float32(np.pi / 2)) / 2
            q0 = [np.cos(h), 0.0, 0.0, np.sin(h)]
            dq = [nc.TRIG_ULP * nc._spacing(q0[0]), 0.0, 0.0, nc.TRIG_ULP * nc._spacing(q0[3])]
            dq = nc._qmul_bound(pose[7:11], nc._qmul(pose[0:4], q0), nc._qmul_bound(pose[0:4], q0, dq))
            assert (np.abs(q - np.array(case["quat"][j])) <= dq).all() and max(dq) < 1e-13, (name, j)
    tilt = np.array(GOLD["tilt"]["velocity"])
    assert (np.abs(tilt[:, 2]) > 0).any()                                          # pitch and roll: the velocity leaves the plane


def test_dets_to_nusc_records_and_the_filter():
    case = GOLD["yaw"]
    boxes = np.array(case["boxes"], np.float32)
    n = len(boxes)
    dets = np.zeros((1, n + 2, 11), np.float32)
    dets[0, :n, :9], dets[0, :n, 9], dets[0, :n, 10] = boxes, np.linspace(0.2, 0.9, n), np.arange(n) % 10
    recs = ne.dets_to_nusc(dets, [n], [dict(cs_rotation=case["pose"][0:4], cs_translation=case["pose"][4:7], ego_rotation=case["pose"][7:11],
                                            ego_translation=case["pose"][11:14])], nc.CLASSES, tokens=["tok"])
    assert len(recs) == n and all(r["sample_token"] == "tok" for r in recs)
    for j, r in enumerate(recs):
        assert r["translation"] == case["center"][j] and r["size"] == case["size"][j] and r["velocity"] == case["velocity"][j][:2]
        assert r["detection_name"] == nc.CLASSES[j % 10] and r["detection_score"] == float(dets[0, j, 9])
        speed = np.sqrt(r["velocity"][0] ** 2 + r["velocity"][1] ** 2)
        mv, st = ne.attr_tables(nc.CLASSES)
        assert r["attribute_name"] == ne.ATTRIBUTES[(mv if speed > 0.2 else st)[j % 10]]
    ego = {"tok": case["pose"][11:14]}
    ev = ne.NuscDetectionEval([], recs, ego, nc.CLASSES)
    dist = np.array([np.hypot(r["translation"][0] - ego["tok"][0], r["translation"][1] - ego["tok"][1]) for r in recs])
    keep = [j for j, r in enumerate(recs) if dist[j] < ne.DETECTION_CVPR_2019["class_range"][r["detection_name"]]]
    assert 0 < len(keep) < n and sorted(ev.z["dt_gidx"].tolist()) == keep
    gt = dict(recs[keep[0]], num_pts=0)
    assert len(ne.NuscDetectionEval([gt, dict(gt, num_pts=2)], recs, ego, nc.CLASSES).z["gt_yaw"]) == 1
