"""Golden vectors for the nuScenes result formatting, produced BY THE REFERENCE's own two routines: _second_det_to_nusc_box and
_lidar_nusc_box_to_global (minddet/models/centerpoint/det3d_ms/datasets/nuscenes/nusc_common.py:160-201).  nusc_common.py is loaded as
a file; what it imports and what is not installable here is stubbed below, minimally: pyquaternion.Quaternion (four elements or
axis + radians, the Hamilton product, the rotation matrix of the normalised quaternion), tqdm, the devkit's Box (centre, size,
orientation, velocity, rotate, translate -- the devkit's statements, with the matrix-vector product written out in the order
minddet_amd/nusc_eval.py documents) and a `nusc` whose get() returns the calibrated_sensor and ego_pose records of the case.  So the
reference supplies the order of the steps (the float32 yaw, the quaternion about z, rotate / translate twice) and the stubs the
arithmetic of a step.  Run here only:

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/gen_nusc_rows.py <path of the reference checkout>

Nothing of the reference is copied: tests/golden/nusc_rows_vectors.json holds seeded float32 boxes, three poses (yaw only, general
with pitch and roll, not normalised) and what the routines returned (centres, sizes, quaternions, velocities).
"""
import json
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
from gen_cp_targets import PKG, _load  # noqa: E402

OUT = os.path.join(HERE, "nusc_rows_vectors.json")


class Quaternion:
    def __init__(self, *args, axis=None, radians=None):
        if axis is not None:
            a = np.asarray(axis, np.float64)
            a = a / np.sqrt(np.dot(a, a))
            theta = float(radians) / 2.0
            self.q = np.array([math.cos(theta), *(a * math.sin(theta))], np.float64)
        else:
            self.q = np.asarray(args[0].q if isinstance(args[0], Quaternion) else args[0], np.float64).copy()

    @property
    def elements(self):
        return self.q

    def __mul__(self, o):
        aw, ax, ay, az = self.q
        bw, bx, by, bz = o.q
        return Quaternion([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                           aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])

    @property
    def rotation_matrix(self):
        w, x, y, z = self.q
        n = np.sqrt(((w * w + x * x) + y * y) + z * z)
        w, x, y, z = w / n, x / n, y / n, z / n
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], np.float64)


def _matvec(r, v):
    return np.array([(r[i][0] * v[0] + r[i][1] * v[1]) + r[i][2] * v[2] for i in range(3)], np.float64)


class Box:
    def __init__(self, center, size, orientation, label=np.nan, score=np.nan, velocity=(np.nan, np.nan, np.nan), name=None, token=None):
        self.center, self.wlh, self.orientation = np.array(center, np.float64), np.array(size, np.float64), orientation
        self.label, self.score, self.velocity, self.name, self.token = label, score, np.array(velocity, np.float64), name, token

    def translate(self, x):
        self.center += x

    def rotate(self, quaternion):
        self.center = _matvec(quaternion.rotation_matrix, self.center)
        self.orientation = quaternion * self.orientation
        self.velocity = _matvec(quaternion.rotation_matrix, self.velocity)


class Nusc:
    def __init__(self, pose):
        self.pose = pose

    def get(self, table, token):
        if table == "sample":
            return {"data": {"LIDAR_TOP": token}}
        if table == "sample_data":
            return {"calibrated_sensor_token": token, "ego_pose_token": token}
        if table == "calibrated_sensor":
            return {"rotation": self.pose[0:4], "translation": self.pose[4:7]}
        return {"rotation": self.pose[7:11], "translation": self.pose[11:14]}


def reference_nusc_common(ref_root):
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        m.__dict__.update(attrs)
        sys.modules[name] = m
    mod("pyquaternion", Quaternion=Quaternion)
    mod("tqdm", tqdm=lambda it, *a, **k: it)
    mod("nuscenes", NuScenes=object)
    for name in ("nuscenes.eval", "nuscenes.eval.detection"):
        mod(name)
    mod("nuscenes.eval.detection.config", config_factory=None)
    mod("nuscenes.eval.detection.evaluate", NuScenesEval=None)
    mod("nuscenes.utils", splits=None)
    mod("nuscenes.utils.data_classes", Box=Box)
    mod("nuscenes.utils.geometry_utils", transform_matrix=None)
    return _load("ref_nusc_common", os.path.join(ref_root, PKG, "datasets/nuscenes/nusc_common.py"))


def main(ref_root):
    nc = reference_nusc_common(ref_root)
    rng = np.random.default_rng(5)
    yaw_q = lambda a: [math.cos(a / 2), 0.0, 0.0, math.sin(a / 2)]
    poses = {"yaw": yaw_q(0.02) + [0.94, 0.0, 1.84] + yaw_q(-2.1) + [411.3, 1180.9, 0.0],
             "tilt": [0.7, 0.012, -0.021, 0.713] + [1.0, 0.1, 1.8] + [0.883, 0.021, 0.034, -0.468] + [600.1, 1600.7, 1.5],
             "scaled": [1.4, 0.0, 0.0, 1.43] + [0.9, 0.0, 1.9] + [-0.6, 0.02, 0.0, 1.9] + [1318.2, 922.4, 0.3]}
    out = {}
    for name, pose in poses.items():
        n = 14
        box = np.zeros((n, 9), np.float32)
        box[:, :2] = rng.uniform(-50, 50, (n, 2))
        box[:, 2] = rng.uniform(-3, 1, n)
        box[:, 3:6] = rng.uniform(0.3, 12, (n, 3))
        box[:, 6:8] = rng.uniform(-8, 8, (n, 2)) * (rng.random((n, 1)) < 0.7)
        box[:, 8] = rng.uniform(-3.2, 3.2, n)
        box[0, 8], box[1, 8] = np.float32(-np.pi / 2), np.float32(np.pi)
        det = {"box3d_lidar": box.copy(), "scores": rng.uniform(0.1, 1, n).astype(np.float32), "label_preds": rng.integers(0, 10, n)}
        boxes = nc._lidar_nusc_box_to_global(Nusc(pose), nc._second_det_to_nusc_box(det), "t")
        assert np.array_equal(det["box3d_lidar"][:, 8], -box[:, 8] - np.float32(np.pi / 2)) and det["box3d_lidar"].dtype == np.float32
        out[name] = dict(pose=[float(v) for v in pose], boxes=box.astype(np.float64).tolist(), center=[b.center.tolist() for b in boxes],
                         size=[b.wlh.tolist() for b in boxes], quat=[b.orientation.elements.tolist() for b in boxes],
                         velocity=[b.velocity.tolist() for b in boxes])
    with open(OUT, "w") as f:
        json.dump(out, f)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
