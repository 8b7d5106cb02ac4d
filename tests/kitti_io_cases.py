"""What tests/test_kitti_io_cpu.py, tests/test_kitti_io_gpu.py and tools/pointpillars_kitti_io_step.py share about the KITTI camera-frame
ends: the fixture (tests/golden/kitti_io_vectors.npz, written by tests/golden/gen_kitti_io.py from the reference's own routines), the
calibrations as det_ops.KittiCalibration, seeded clouds, hulls and detections."""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kitti_io_vectors.npz")
f = np.float32


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


def calibration(which=(0,), device="cpu"):
    """det_ops.KittiCalibration of the fixture's calibrations `which` (one batch entry each)"""
    from minddet_amd import det_ops

    z = fixture()
    return det_ops.KittiCalibration(*[np.stack([z[f"cal{c}_{k}"] for c in which]) for k in ("rect", "trv2c", "p2", "image_shape")], device=device)


def scan(seed, n, reach=75.0, zlo=-3.0, zhi=1.5):
    """[n,4] fp32: a full turn of the scanner"""
    rng = np.random.default_rng(seed)
    r, th = rng.uniform(2, reach, n), rng.uniform(-np.pi, np.pi, n)
    return np.stack([r * np.cos(th), r * np.sin(th), rng.uniform(zlo, zhi, n), rng.uniform(0, 1, n)], 1).astype(f)


def boxes_as_hulls(rng, B, K, span=30.0):
    """[B,K,8,3] f64: upright boxes of random yaw as eight corners in the order of the reference's corner functions
    (center_to_corner_box3d: the unravelled 2x2x2 index with the swap [0, 1, 3, 2, 4, 5, 7, 6]), whose surfaces' normals point inwards"""
    unit = np.stack(np.unravel_index(np.arange(8), [2] * 3), 1)[[0, 1, 3, 2, 4, 5, 7, 6]].astype(np.float64) - 0.5
    out = np.zeros((B, K, 8, 3))
    for b in range(B):
        for k in range(K):
            dims, yaw = rng.uniform(4, 25, 3) * (1, 1, 0.3), rng.uniform(-np.pi, np.pi)
            c, s = np.cos(yaw), np.sin(yaw)
            p = unit * dims
            out[b, k] = np.stack([p[:, 0] * c - p[:, 1] * s, p[:, 0] * s + p[:, 1] * c, p[:, 2]], 1) + (rng.uniform(-span, span), rng.uniform(-span, span), -1.0)
    return out


def detections(seed, B, M, calib, spread=1.0):
    """dets [B,M,9] fp32 in front of the camera of `calib`, well inside the image and the car range: x 8 .. 50, |y| < 0.25 x, KITTI sizes"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(8, 50, (B, M))
    d = np.stack([x, rng.uniform(-0.25, 0.25, (B, M)) * x * spread, rng.uniform(-1.6, -0.6, (B, M)), rng.uniform(1.4, 1.9, (B, M)),
                  rng.uniform(3.2, 4.6, (B, M)), rng.uniform(1.3, 1.9, (B, M)), rng.uniform(-np.pi, np.pi, (B, M)), rng.uniform(0.1, 1, (B, M)),
                  rng.integers(0, 3, (B, M)).astype(np.float64)], -1)
    return d.astype(f)


CAR_RANGE = [0, -39.68, -5, 69.12, 39.68, 5]
