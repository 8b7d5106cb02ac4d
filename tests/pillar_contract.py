"""The point-cloud front end's contract (include/minddet_hip_points.h) written out in numpy.

voxelize_loop / voxelize_ref: md_voxelize.  The first is the sequential statement (one Python loop over the points, the order the header
refers to), for small clouds; the second computes the same from order-free facts with numpy sorts, for production-size clouds.  Both do
the cell arithmetic in fp32 exactly as the header says: fp32 subtract, fp32 divide, floor.  tests/test_pillars_cpu.py holds them
against each other and against the fixture the reference's own points_to_voxel produced (tests/golden/pillar_vectors.npz).

pfn_ref: md_pillar_encode in float64, per voxel row, together with a bound on what the fp32 operation sequence of the header may differ
from it.  The bound is carried through the sequence, with u = 2^-24 (half an ulp, relative) per rounding point:
  add / sub   |fl(a + b) - (a + b)| <= ea + eb + u (|a + b| + ea + eb)            for inputs known to within ea, eb
  mul         <= |a| eb + |b| ea + ea eb + u (|a b| + the same)
  divide by n exact n: <= ea / n + u (|a| + ea) / n
  sum, dot    n terms in any order, FMA or not: <= gamma(n) sum |terms|, gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability of
              Numerical Algorithms, 3.1 / 3.5); a layer is a dot product of K terms plus the shift (plus, in layer 2, the join of its
              two halves): gamma(K + 2) over sum |w| |x| + |shift|, K = F + 5 and K = 64; on top the inputs' own error sum |w| ex
  relu, max   monotone and 1-Lipschitz: the bound passes through (the maximum of the rows' bounds)
  bf16 store  round to nearest even of a value within the bound of the float64 one: it may land on either neighbour when the float64
              value lies within the bound of a rounding midpoint -- bf16_interval gives the admissible results."""
import numpy as np

U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


# ------------------------------------------------------------------------------------------------------------------------ voxeliser
def grid_of(voxel_size, pc_range):
    vs, r = np.asarray(voxel_size, np.float32), np.asarray(pc_range, np.float32)
    return np.round((r[3:] - r[:3]) / vs).astype(np.int32)          # (gx, gy, gz), fp32 like the reference


def cells_of(points, voxel_size, pc_range, reciprocal=False):
    """-> (cell [n, 3] int64 as (x, y, z), valid [n]) in fp32.  reciprocal=True is the WRONG form the header excludes (tests show that
    the data can tell them apart)."""
    vs, r = np.asarray(voxel_size, np.float32), np.asarray(pc_range, np.float32)
    xyz = points[:, :3].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = xyz - r[:3]
        c = np.floor(d * (np.float32(1) / vs) if reciprocal else d / vs)
        g = grid_of(voxel_size, pc_range).astype(np.float32)
        valid = np.isfinite(xyz).all(1) & (c >= 0).all(1) & (c < g).all(1)
    return np.where(valid[:, None], c, 0).astype(np.int64), valid


def voxelize_loop(points, offsets, voxel_size, pc_range, max_points, max_voxels):
    """the sequential statement: per sample, points in index order"""
    B, F = len(offsets) - 1, points.shape[1]
    voxels = np.zeros((B, max_voxels, max_points, F), np.float32)
    coors = np.zeros((B, max_voxels, 4), np.int32)
    num = np.zeros((B, max_voxels), np.int32)
    vnum = np.zeros((B,), np.int32)
    cell, valid = cells_of(points, voxel_size, pc_range)
    for b in range(B):
        seen = {}
        for i in range(int(offsets[b]), int(offsets[b + 1])):
            if not valid[i]:
                continue
            key = (int(cell[i, 2]), int(cell[i, 1]), int(cell[i, 0]))
            v = seen.get(key)
            if v is None:
                if vnum[b] >= max_voxels:
                    continue
                v = seen[key] = int(vnum[b])
                vnum[b] += 1
                coors[b, v] = (b,) + key
            if num[b, v] < max_points:
                voxels[b, v, num[b, v]] = points[i]
                num[b, v] += 1
    return voxels, coors, num, vnum


def voxelize_ref(points, offsets, voxel_size, pc_range, max_points, max_voxels):
    """the same result without a loop over the points"""
    B, F = len(offsets) - 1, points.shape[1]
    gx, gy, gz = (int(v) for v in grid_of(voxel_size, pc_range))
    voxels = np.zeros((B, max_voxels, max_points, F), np.float32)
    coors = np.zeros((B, max_voxels, 4), np.int32)
    num = np.zeros((B, max_voxels), np.int32)
    vnum = np.zeros((B,), np.int32)
    cell, valid = cells_of(points, voxel_size, pc_range)
    for b in range(B):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        idx = lo + np.nonzero(valid[lo:hi])[0]                      # index order
        if idx.size == 0 or max_voxels == 0:
            continue
        cid = (cell[idx, 2] * gy + cell[idx, 1]) * gx + cell[idx, 0]
        uniq, first, inv = np.unique(cid, return_index=True, return_inverse=True)
        rank_of_uniq = np.empty(len(uniq), np.int64)
        rank_of_uniq[np.argsort(first, kind="stable")] = np.arange(len(uniq))   # voxels numbered by their first point
        vnum[b] = min(len(uniq), max_voxels)
        kept_u = rank_of_uniq < max_voxels
        c = uniq[kept_u]
        coors[b, rank_of_uniq[kept_u]] = np.stack([np.full_like(c, b), c // (gx * gy), c // gx % gy, c % gx], 1)
        vox = rank_of_uniq[inv.reshape(-1)]
        keep = vox < max_voxels
        idx, vox = idx[keep], vox[keep]
        order = np.argsort(vox, kind="stable")                      # by voxel, index order inside
        idx, vox = idx[order], vox[order]
        start = np.searchsorted(vox, vox, side="left")
        slot = np.arange(len(vox)) - start
        cnt = np.bincount(vox, minlength=max_voxels)[:max_voxels]
        num[b] = np.minimum(cnt, max_points)
        take = slot < max_points
        voxels[b, vox[take], slot[take]] = points[idx[take]]
    return voxels, coors, num, vnum


# ------------------------------------------------------------------------------------------------------------------- pillar encoder
def _add(a, ea, b, eb, sign=1.0):
    v = a + sign * b
    e = ea + eb
    return v, e + U * (np.abs(v) + e)


def _mul(a, ea, b, eb):
    v = a * b
    e = np.abs(a) * eb + np.abs(b) * ea + ea * eb
    return v, e + U * (np.abs(v) + e)


def _layer(x, ex, w, b):
    """rows x [..., K] (known to within ex) -> relu(w x + b), its bound"""
    w, b = w.astype(np.float64), b.astype(np.float64)
    K = w.shape[1]
    v = x @ w.T + b
    mag = (np.abs(x) + ex) @ np.abs(w).T + np.abs(b)
    e = ex @ np.abs(w).T + gamma(K + 2) * mag
    return np.maximum(v, 0.0), e


def pfn_ref(voxels, num_points, coors, voxel_num, *args, chunk=2048, **kw):
    """_pfn_rows over the voxel rows in chunks (the float64 intermediates of 60 000 x 20 rows do not have to exist at once)"""
    MV = voxels.shape[1]
    parts = [_pfn_rows(voxels[:, i:i + chunk], num_points[:, i:i + chunk], coors[:, i:i + chunk], voxel_num, i, *args, **kw)
             for i in range(0, max(MV, 1), chunk)]
    return tuple(np.concatenate([p[k] for p in parts], 1) for k in range(3))


def _pfn_rows(voxels, num_points, coors, voxel_num, row0, w1, b1, w2, b2, vx, vy, x_offset, y_offset, skip_padded=False, swap_xy=False):
    """-> (feat [B, MV, 64] float64, bound [B, MV, 64], live [B, MV] bool): what md_pillar_encode writes at (coors.b, coors.y, coors.x)
    for every row v < voxel_num[b] (live), before the bf16 store.  skip_padded / swap_xy are two WRONG forms (padded rows left out of
    the maximum; x and y swapped in the centre offset) for the tests that show the data can see those mistakes."""
    B, MV, MP, F = voxels.shape
    p = voxels.astype(np.float64)
    n = np.clip(num_points.astype(np.int64), 0, MP)
    live = row0 + np.arange(MV)[None, :] < voxel_num.astype(np.int64)[:, None]
    rowmask = np.arange(MP)[None, None, :] < n[:, :, None]                                 # the padding mask
    p = p * rowmask[..., None]
    nn_ = np.maximum(n, 1).astype(np.float64)[..., None]
    # mean: sequential sum of n exact terms, then the divide
    s = p[..., :3].sum(2)
    es = gamma(MP) * np.abs(p[..., :3]).sum(2)
    mean = s / nn_
    emean = es / nn_ + U * (np.abs(s) + es) / nn_
    fc, efc = _add(p[..., :3], 0.0, mean[:, :, None, :], emean[:, :, None, :], -1.0)
    cx, cy = coors[..., 3].astype(np.float64), coors[..., 2].astype(np.float64)
    if swap_xy:
        cx, cy = cy, cx
    tx, etx = _mul(cx, 0.0, np.float64(np.float32(vx)), 0.0)
    tx, etx = _add(tx, etx, np.float64(np.float32(x_offset)), 0.0)
    ty, ety = _mul(cy, 0.0, np.float64(np.float32(vy)), 0.0)
    ty, ety = _add(ty, ety, np.float64(np.float32(y_offset)), 0.0)
    fx, efx = _add(p[..., 0], 0.0, tx[..., None], etx[..., None], -1.0)
    fy, efy = _add(p[..., 1], 0.0, ty[..., None], ety[..., None], -1.0)
    x = np.concatenate([p, fc, fx[..., None], fy[..., None]], -1) * rowmask[..., None]
    ex = np.concatenate([np.zeros_like(p), efc, efx[..., None], efy[..., None]], -1) * rowmask[..., None]   # padded rows are exact zeros

    def row_max(y, ey):
        """max over the MP rows; the padded rows are in y already (their input is zero) unless skip_padded"""
        if skip_padded:
            y = np.where(rowmask[..., None], y, -np.inf)
        m = y.max(2)
        return np.where(np.isfinite(m), m, 0.0), np.where(rowmask[..., None] | (not skip_padded), ey, 0.0).max(2)

    y, ey = _layer(x, ex, w1, b1)
    m, em = row_max(y, ey)
    if w2 is not None:
        x2 = np.concatenate([y, np.broadcast_to(m[:, :, None, :], y.shape)], -1)
        ex2 = np.concatenate([ey, np.broadcast_to(em[:, :, None, :], ey.shape)], -1)
        y, ey = _layer(x2, ex2, w2, b2)
        m, em = row_max(y, ey)
    empty = (n <= 0)[..., None]                                                           # the voxel mask: zeros
    m, em = np.where(empty, 0.0, m), np.where(empty, 0.0, em)
    return m, em * (1 + 1e-9) + 1e-300, live


def bf16_round(x):
    """float64 -> the nearest bf16 value (ties to even), as float64; normal range"""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)
    q = np.ldexp(1.0, np.maximum(e, -125) - 8)           # spacing of bf16 (8 significant bits) at x
    return np.rint(x / q) * q


def bf16_interval(ref, bound):
    """the bf16 results a correctly rounded store of any value within `bound` of `ref` can give (rounding is monotone)"""
    return bf16_round(ref - bound), bf16_round(ref + bound)
