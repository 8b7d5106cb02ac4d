"""The KITTI reader's contract (include/minddet_hip_ppreader.h, md_pp_pillar_encode) written out in numpy, as tests/pillar_contract.py
does for md_pillar_encode.

The inputs of the Dense are bit-defined, so `features` computes them exactly: fp32 numpy operations in the header's order (numpy rounds
every operation once and never contracts), then `.astype(np.float16)` (round to nearest even); the weights likewise.  From there on the
header leaves the summation order open, so `interval` carries an interval through the rest:
  Dense   the products of fp16 values are exact; their sum in float64, +- gamma(16) sum |terms| for any fp32 order (u = 2^-24; Higham,
          Accuracy and Stability of Numerical Algorithms, 3.1): [lo, hi] -> the fp16 results a rounding of anything in that range can give
          (rounding is monotone: the roundings of the two ends)
  affine  scale * d + shift in fp32, as one FMA or as two roundings: at both ends of d's range (monotone in d), +- u |scale d| (1 + u)
          + u |value|; a zero product adds nothing (the shift comes back as it is)
  fp16    again the roundings of the two ends; ReLU and the maximum over the rows are monotone; so is the bf16 store
A device value passes if it lies in [lo, hi].  `emulate` is one admissible device (fp32 accumulation in k order) -- and, with `wrong=`,
one of six devices the header excludes; tests/test_pp_reader_cpu.py shows that the data tells each of them from the contract."""
import numpy as np

from tests.pillar_contract import U, bf16_round, gamma

WRONG = ("inputs_not_fp16", "weights_not_fp16", "dense_not_fp16", "bn_not_fp16", "bn_folded_into_weights", "no_z_centre")


def features(voxels, num_points, coors, voxel_size, offsets, with_distance=False, no_z_centre=False):
    """-> f [B, MV, MP, K] float32, bit-defined; rows >= clamp(num_points, 0, MP) are zero"""
    B, MV, MP, F = voxels.shape
    assert F == 4
    p = voxels.astype(np.float32)
    n = np.clip(num_points.astype(np.int64), 0, MP)
    rows = np.arange(MP)[None, None, :] < n[:, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros((B, MV, 3), np.float32)
        for r in range(MP):                                  # the fp32 sum in row order, over the n points only
            s = np.where(rows[:, :, r, None], s + p[:, :, r, :3], s)
        mean = s / np.maximum(n, 1).astype(np.float32)[..., None]
        vs, off = np.asarray(voxel_size, np.float32), np.asarray(offsets, np.float32)
        ctr = [coors[..., 3 - k].astype(np.float32) * vs[k] + off[k] for k in range(3)]      # x from coors.x, y from coors.y, z from coors.z
        cols = [p[..., 0], p[..., 1], p[..., 2], p[..., 3]]
        cols += [p[..., k] - mean[:, :, None, k] for k in range(3)]
        cols += [p[..., k] - ctr[k][..., None] for k in range(3)]
        if no_z_centre:
            cols[9] = np.zeros_like(cols[9])
        if with_distance:
            cols.append(np.sqrt((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2]))
        f = np.stack(cols, -1).astype(np.float32)
    return np.where(rows[..., None], f, np.float32(0))


def _f16(x):
    with np.errstate(over="ignore"):
        return np.asarray(x).astype(np.float16).astype(np.float64)


def interval(voxels, num_points, coors, voxel_num, w, scale, shift, voxel_size, offsets, with_distance=False, chunk=512):
    """-> (lo [B, MV, 64], hi [B, MV, 64] float64: the admissible bf16 results, live [B, MV] bool)"""
    B, MV, MP, _ = voxels.shape
    w16 = _f16(w.astype(np.float32))                                                        # [64, K]
    sc, sh = scale.astype(np.float64), shift.astype(np.float64)
    lo, hi = np.zeros((B, MV, 64)), np.zeros((B, MV, 64))
    for i in range(0, MV, chunk):
        f = features(voxels[:, i:i + chunk], num_points[:, i:i + chunk], coors[:, i:i + chunk], voxel_size, offsets, with_distance)
        a16 = _f16(f)                                                                      # [B, c, MP, K]
        dot = a16 @ w16.T
        e = gamma(16) * (np.abs(a16) @ np.abs(w16).T)
        ends = []
        for d in (_f16(dot - e), _f16(dot + e)):
            prod = sc * d
            v = prod + sh
            e2 = U * np.abs(prod) * (1 + U) + np.where(prod != 0, U * np.abs(v), 0.0)
            ends.append((_f16(v - e2), _f16(v + e2)))
        ylo = np.minimum(ends[0][0], ends[1][0])
        yhi = np.maximum(ends[0][1], ends[1][1])
        lo[:, i:i + chunk] = bf16_round(np.maximum(ylo, 0.0).max(2))
        hi[:, i:i + chunk] = bf16_round(np.maximum(yhi, 0.0).max(2))
    live = np.arange(MV)[None, :] < voxel_num.astype(np.int64)[:, None]
    return lo, hi, live


def emulate(voxels, num_points, coors, w, scale, shift, voxel_size, offsets, with_distance=False, wrong=None):
    """one device: fp32 accumulation in k order, the affine as two fp32 roundings -> [B, MV, 64] float64 (bf16 values).  wrong: one of
    WRONG, a device the header excludes."""
    assert wrong is None or wrong in WRONG
    f = features(voxels, num_points, coors, voxel_size, offsets, with_distance, no_z_centre=wrong == "no_z_centre")
    f32 = np.float32
    w = w.astype(f32)
    if wrong == "bn_folded_into_weights":
        w = w * scale.astype(f32)[:, None]
    with np.errstate(over="ignore"):
        a = f if wrong == "inputs_not_fp16" else f.astype(np.float16).astype(f32)
        wk = w if wrong == "weights_not_fp16" else w.astype(np.float16).astype(f32)
        acc = np.zeros(f.shape[:3] + (64,), f32)
        for k in range(f.shape[3]):
            acc = acc + a[..., k, None] * wk[None, None, None, :, k]
        d = acc if wrong == "dense_not_fp16" else acc.astype(np.float16).astype(f32)
        y = d + shift.astype(f32) if wrong == "bn_folded_into_weights" else scale.astype(f32) * d + shift.astype(f32)
        y = y if wrong == "bn_not_fp16" else y.astype(np.float16).astype(f32)
    return bf16_round(np.maximum(y, 0).max(2).astype(np.float64))


def car_like_voxels(seed, B=2, MV=1200, MP=32, hw=(496, 432), voxel_size=(0.16, 0.16, 4.0), pc_range=(0, -39.68, -3, 69.12, 39.68, 1),
                    dead_garbage=True):
    """voxels as md_voxelize leaves them on the Car grid: points inside their pillar, z over the range, reflectance in [0, 1); counts
    1, MP - 1 and MP among them, one live row with a hand-set count of 0; distinct cells per sample; sample 1 has MV // 2 live rows;
    rows past voxel_num hold garbage, a few live rows have coors outside the canvas.  -> voxels, num_points, coors, voxel_num"""
    rng = np.random.default_rng(seed)
    H, W = hw
    voxel_num = np.array([MV if b != 1 else MV // 2 for b in range(B)], np.int32)
    num = np.minimum(rng.geometric(0.25, (B, MV)), MP).astype(np.int32)
    num[:, 0], num[:, 1], num[:, 2], num[:, 3] = 1, MP - 1, MP, 0
    coors = np.zeros((B, MV, 4), np.int32)
    for b in range(B):
        cell = rng.permutation(H * W)[:MV]
        coors[b] = np.stack([np.full(MV, b), np.zeros(MV, np.int64), cell // W, cell % W], 1)
    vx, vy, vz = voxel_size
    shape = (B, MV, MP)
    voxels = np.stack([pc_range[0] + (coors[..., 3:4] + rng.uniform(0, 1, shape)) * vx, pc_range[1] + (coors[..., 2:3] + rng.uniform(0, 1, shape)) * vy,
                       rng.uniform(pc_range[2], pc_range[2] + vz, shape), rng.uniform(0, 1, shape)], -1).astype(np.float32)
    voxels *= (np.arange(MP)[None, None, :, None] < num[..., None, None])
    coors[:, 5, 2], coors[:, 6, 3], coors[:, 7, 2] = H, -1, -3                              # outside the canvas: nothing is written
    if dead_garbage:
        dead = np.arange(MV)[None, :] >= voxel_num[:, None]
        voxels[dead] = rng.normal(0, 50, voxels[dead].shape).astype(np.float32)
        num[dead] = rng.integers(-5, 2 * MP, num[dead].shape)
        coors[dead] = rng.integers(0, min(H, W), coors[dead].shape)
    return voxels, num, coors, voxel_num


def random_reader(seed, K=10):
    """-> (w [64, K], scale [64], shift [64]) float32: weights N(0, 2 / K), scales of both signs, shifts of both signs"""
    rng = np.random.default_rng(seed)
    w = rng.normal(0, np.sqrt(2.0 / K), (64, K)).astype(np.float32)
    scale = (rng.uniform(0.5, 1.5, 64) / np.sqrt(rng.uniform(0.5, 1.5, 64) + 1e-3)).astype(np.float32)
    scale[::9] *= -1                                                                          # a negative gamma: the smallest d wins
    shift = rng.normal(0.1, 0.5, 64).astype(np.float32)
    return w, scale, shift
