"""The three operators of include/minddet_hip_kitti.h stated in numpy float64, with the margin of every decision, and the forward
bound between the all-float64 result rows and minddet_amd/kitti_eval.py's host path.

Arithmetic: every value is float64 made from the fp32 inputs and the float64 matrices; a sum is taken from the left, term by term
(numpy evaluates an expression like ((a * b + c * d) + e * f) + g exactly so, one rounding per operation, nothing fused), which is what
csrc/kitti.hip does without contraction.  So the device's decisions and float64 values are the contract's bit for bit, up to sincos
and atan2 (the device's and numpy's are both within a few ulp of float64); an fp32 output is fp32(contract) except where such a
difference crosses an fp32 rounding boundary: at most 1 in 10^4 values off by one ulp is allowed, as for the losses.

Margins (what "open" means below: a decision that another evaluation order of the same formula could take the other way)
  plane sign    sign = ((px n0 + py n1) + pz n2) + d is open when |sign| <= SIGN_ULPS * 2^-53 * (|px n0| + |py n1| + |pz n2| + |d|): three
                additions and three products round once each, a different order or a fused product moves the sum by at most 4 ulp of
                the term sum; the reference's d comes out of np.einsum, whose order numpy does not promise; 64 ulp leaves room
  image box     x1 > W, y1 > H, x2 < 0, y2 < 0 are open when the value lies within `uv_err` of its threshold: uv_err is the rounding of
                u = (p X + ...) / Z in float64, UV_ULPS * 2^-53 * (|p00 X| + |p01 Y| + |p02 Z| + |p03|) / |Z| plus the same relative
                share of |u| for Z's own rounding (the corner sums before it are three operations deep)
  range         the six comparisons read the fp32 centre and the fp32 limits widened to float64: no arithmetic, never open
"""
import numpy as np

U = 2.0 ** -53          # unit roundoff of float64
U32 = 2.0 ** -24        # of fp32
SIGN_ULPS = 64
UV_ULPS = 64
FEW = 1e-4              # share of fp32 outputs that may sit one ulp from fp32(contract)
MAX_HULLS, MAX_DETS = 64, 512
SURFACES = np.array([0, 1, 2, 3, 7, 6, 5, 4, 0, 3, 7, 4, 1, 5, 6, 2, 0, 4, 5, 1, 3, 2, 6, 7]).reshape(6, 4)      # box_np_ops.py:735-737
ROW_NAMES = ("alpha", "x1", "y1", "x2", "y2", "l", "h", "w", "x", "y", "z", "rotation_y", "score", "label")


# ----------------------------------------------------------------------------- md_pc_crop_hulls
def planes(hulls):
    """hulls [..., 8, 3] f64 -> [..., 6, 4]: (n0, n1, n2, d) of surface_equ_3d_jit over corner_to_surfaces_3d_jit"""
    hulls = np.asarray(hulls, np.float64)
    s0, s1, s2 = (hulls[..., SURFACES[:, k], :] for k in range(3))
    a, b = s0 - s1, s1 - s2
    n0 = a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
    n1 = a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
    n2 = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    d = -((n0 * s0[..., 0] + n1 * s0[..., 1]) + n2 * s0[..., 2])
    return np.stack([n0, n1, n2, d], -1)


def signs(points, pl):
    """points [n, >=3] f32, pl [K, 6, 4] -> (sign [n, K, 6], margin [n, K, 6])"""
    p = np.asarray(points, np.float32)[:, None, None, :3].astype(np.float64)
    t0, t1, t2 = p[..., 0] * pl[None, ..., 0], p[..., 1] * pl[None, ..., 1], p[..., 2] * pl[None, ..., 2]
    d = np.broadcast_to(pl[None, ..., 3], t0.shape)
    with np.errstate(invalid="ignore"):
        s = ((t0 + t1) + t2) + d
        return s, SIGN_ULPS * U * (np.abs(t0) + np.abs(t1) + np.abs(t2) + np.abs(d))


def inside(points, hulls):
    """-> (mask [n, K] as points_in_convex_polygon_3d_jit gives it, open [n, K])"""
    s, m = signs(points, planes(hulls))
    with np.errstate(invalid="ignore"):
        out = s >= 0
        near = np.abs(s) <= m
    mask = ~out.any(-1)
    # a hull is left at its first non-negative sign: only an open sign that could change the outcome counts
    open_ = (near & ~(out & ~near).any(-1, keepdims=True)).any(-1)
    return mask, open_


def crop_hulls(points, offsets, hulls, hull_count):
    """points [N,4] f32, offsets [B+1], hulls [B,K,8,3] f64, hull_count [B] -> dict(points [N,4] f32 with the zero tail, offsets [B+1]
    i32, keep [N] u8, src [kept] the input rows in output order, open [N] bool)"""
    points = np.ascontiguousarray(points, np.float32)
    N, B = len(points), len(offsets) - 1
    K = hulls.shape[1]
    offs = np.clip(np.asarray(offsets, np.int64), 0, N)
    keep, open_ = np.zeros(N, np.uint8), np.zeros(N, bool)
    for b in range(B):
        lo, hi = int(offs[b]), int(offs[b + 1])
        cnt = int(min(max(int(hull_count[b]), 0), K))
        if hi <= lo or cnt == 0:
            continue
        mask, op = inside(points[lo:hi], hulls[b, :cnt])
        keep[lo:hi] = mask.any(-1)
        sure = (mask & ~op).any(-1)              # inside a hull for certain: the other hulls' open signs change nothing
        open_[lo:hi] = op.any(-1) & ~sure
    src = np.flatnonzero(keep)
    out = np.zeros_like(points)
    out[:len(src)] = points[src]
    csum = np.concatenate([[0], np.cumsum(keep)])
    return dict(points=out, offsets=csum[offs].astype(np.int32), keep=keep, src=src, open=open_)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_crop(got_points, got_offsets, got_keep, c, what=""):
    """exact: keep, the order, offsets_out, every column of the kept rows and the zero tail"""
    assert not c["open"].any(), (what, "the case has open decisions", np.flatnonzero(c["open"])[:8])
    assert np.array_equal(got_keep, c["keep"]), (what, "keep", np.flatnonzero(got_keep != c["keep"])[:8])
    assert np.array_equal(got_offsets, c["offsets"]), (what, got_offsets, c["offsets"])
    assert same_bits(got_points, c["points"]), (what, "points")


# ----------------------------------------------------------------------------- md_kitti_boxes_to_lidar
def apply4(m, xyz):
    """rows 0-2 of m @ [x, y, z, 1], from the left: m [..., 4, 4], xyz [..., n, 3] f64 -> [..., n, 3]"""
    m = np.asarray(m, np.float64)[..., None, :, :]
    x, y, z = xyz[..., 0:1], xyz[..., 1:2], xyz[..., 2:3]
    return ((m[..., :3, 0] * x + m[..., :3, 1] * y) + m[..., :3, 2] * z) + m[..., :3, 3]


def boxes_to_lidar(boxes_cam, gt_count, cam2lidar):
    """boxes_cam [B,G,7] f32, gt_count [B], cam2lidar [B,4,4] f64 -> (boxes [B,G,7] f32, xyz [B,G,3] f64 before the store)"""
    q = np.asarray(boxes_cam, np.float32)
    B, G = q.shape[:2]
    xyz = apply4(cam2lidar, q[..., :3].astype(np.float64))
    out = np.concatenate([xyz.astype(np.float32), q[..., 5:6], q[..., 3:4], q[..., 4:5], q[..., 6:7]], -1)
    live = np.arange(G)[None, :] < np.clip(np.asarray(gt_count), 0, G)[:, None]
    return np.where(live[..., None], out, np.float32(0)), xyz


# ----------------------------------------------------------------------------- md_kitti_rows
_SX = np.array([1, 1, -1, -1, 1, 1, -1, -1], np.float64)
_SZ = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.float64)


def camera_rows(dets, lidar2cam, p2):
    """one sample: dets [n,9] f32 -> dict of float64 arrays: loc [n,3], corners [n,8,3], uv [n,8,2], uv_err [n,8,2], bbox [n,4] (before the
    clip), bbox_err [n,4]"""
    q = np.asarray(dets, np.float32).astype(np.float64)
    p2 = np.asarray(p2, np.float64)
    w, l, h, r = q[:, 3:4], q[:, 4:5], q[:, 5:6], q[:, 6:7]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        loc = apply4(lidar2cam, q[:, :3])
        s, c = np.sin(r), np.cos(r)
        xc, zc = _SX[None] * (l / 2), _SZ[None] * (w / 2)
        yc = np.concatenate([np.zeros((len(q), 4)), np.broadcast_to(-h, (len(q), 4))], 1)
        X, Y, Z = (xc * c + zc * s) + loc[:, 0:1], yc + loc[:, 1:2], (-xc * s + zc * c) + loc[:, 2:3]
        uv, err = [], []
        for row in (0, 1):
            t = [p2[row, 0] * X, p2[row, 1] * Y, p2[row, 2] * Z, np.broadcast_to(p2[row, 3], X.shape)]
            num = ((t[0] + t[1]) + t[2]) + t[3]
            uv.append(num / Z)
            err.append(UV_ULPS * U * (sum(np.abs(k) for k in t) / np.abs(Z) + np.abs(num / Z)))
        uv, err = np.stack(uv, -1), np.stack(err, -1)
        bbox = np.concatenate([uv.min(1), uv.max(1)], 1)
        bbox_err = np.concatenate([err.max(1), err.max(1)], 1)
    return dict(loc=loc, corners=np.stack([X, Y, Z], -1), uv=uv, uv_err=err, bbox=bbox, bbox_err=bbox_err)


def kitti_rows(dets, count, lidar2cam, p2, image_shape, limit_range=None, lidar_input=False):
    """dets [B,M,9] f32, count [B], lidar2cam / p2 [B,4,4] f64, image_shape [B,2] (h, w); limit_range: six values taken as fp32 (what the
    attribute struct holds) or None -> dict(rows [B,M,14] f64 (the values before the fp32 store), rows32 [B,M,14] f32, src [B,M] i32,
    count [B] i32, open [B,M] bool indexed like dets, dropped [B,M] bool)"""
    dets = np.asarray(dets, np.float32)
    B, M = dets.shape[:2]
    rows, src = np.zeros((B, M, 14)), np.full((B, M), -1, np.int32)
    open_, dropped, out_count = np.zeros((B, M), bool), np.zeros((B, M), bool), np.zeros(B, np.int32)
    lim = None if limit_range is None else np.asarray(limit_range, np.float32).astype(np.float64)
    for b in range(B):
        n = int(min(max(int(count[b]), 0), M))
        if n == 0:
            continue
        q = dets[b, :n].astype(np.float64)
        g = camera_rows(dets[b, :n], lidar2cam[b], p2[b])
        H, W = float(image_shape[b][0]), float(image_shape[b][1])
        x1, y1, x2, y2 = (g["bbox"][:, k].copy() for k in range(4))
        e = g["bbox_err"]
        drop = np.zeros(n, bool)
        with np.errstate(invalid="ignore"):
            if lim is not None:                  # exact comparisons of inputs: a row the range drops is dropped whatever its image box
                drop |= (q[:, :3] < lim[:3]).any(1) | (q[:, :3] > lim[3:]).any(1)
            if not lidar_input:
                near = (np.abs(x1 - W) <= e[:, 0]) | (np.abs(y1 - H) <= e[:, 1]) | (np.abs(x2) <= e[:, 2]) | (np.abs(y2) <= e[:, 3])
                open_[b, :n] = near & ~drop
                drop |= (x1 > W) | (y1 > H) | (x2 < 0) | (y2 < 0)
            x2, y2 = np.where(W < x2, W, x2), np.where(H < y2, H, y2)
            x1, y1 = np.where(0 > x1, 0.0, x1), np.where(0 > y1, 0.0, y1)
            alpha = -np.arctan2(-q[:, 1], q[:, 0]) + q[:, 6]
        full = np.stack([alpha, x1, y1, x2, y2, q[:, 4], q[:, 5], q[:, 3], g["loc"][:, 0], g["loc"][:, 1], g["loc"][:, 2], q[:, 6], q[:, 7], q[:, 8]], 1)
        kept = np.flatnonzero(~drop)
        rows[b, :len(kept)] = full[kept]
        src[b, :len(kept)] = kept
        out_count[b] = len(kept)
        dropped[b, :n] = drop
    with np.errstate(over="ignore", invalid="ignore"):
        rows32 = rows.astype(np.float32)
    return dict(rows=rows, rows32=rows32, src=src, count=out_count, open=open_, dropped=dropped)


def ulp_steps(a, b):
    """distance in fp32 steps between two fp32 arrays of equal sign pattern; NaN against NaN is 0, +-0 are one value"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    d = np.abs(ia - ib)
    return np.where(np.isnan(a) & np.isnan(b), 0, np.where(np.isnan(a) != np.isnan(b), 1 << 40, d))


def check_stored(got, want32, what=""):
    """fp32 outputs against fp32(contract): equal, at most FEW of them one ulp away -> (differing, total)"""
    steps = ulp_steps(got, want32)
    assert steps.max(initial=0) <= 1, (what, "more than one ulp", int(steps.max()), np.argwhere(steps > 1)[:4].tolist())
    differ, total = int((steps == 1).sum()), steps.size
    assert differ <= max(FEW * total, 0), (what, f"{differ} of {total} stored values are one ulp off")
    return differ, total


def check_rows(got_rows, got_src, got_count, c, what=""):
    assert not c["open"].any(), (what, "the case has open decisions", np.argwhere(c["open"])[:8].tolist())
    assert np.array_equal(got_count, c["count"]), (what, got_count, c["count"])
    assert np.array_equal(got_src, c["src"]), (what, "src")
    return check_stored(got_rows, c["rows32"], what)


# ----------------------------------------------------------------------------- the forward bound to kitti_eval's host path
def host_path_bound(dets, lidar2cam, p2):
    """one sample: the distance allowed between the contract's unclipped image box / location and what
    kitti_eval.lidar_boxes_to_prediction returns for the same dets, derived from that code: camera_box_corners stores the eight
    corners as fp32 (corners.astype(np.float32)), so a corner coordinate moves by at most U32 |coordinate|; then
    u = (p00 X + p01 Y + p02 Z + p03) / Z moves by at most (|p00| dX + |p01| dY + |p02| dZ) / |Z| + |u| dZ / |Z| to first order; the
    factor (1 + 4 U32) / (1 - U32 ...) of the second order is covered by SECOND; the float64 evaluation noise of both sides by uv_err.
    min and max over the corners move by at most the largest corner's share.  The location is float64 on both sides: its sum order only.
    -> (bbox_bound [n,4], loc_bound [n,3])"""
    SECOND = 1.0 + 1e-5
    g = camera_rows(dets, lidar2cam, p2)
    p2 = np.asarray(p2, np.float64)
    X, Y, Z = (np.abs(g["corners"][..., k]) for k in range(3))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        per = []
        for row in (0, 1):
            du = U32 * (abs(p2[row, 0]) * X + abs(p2[row, 1]) * Y + abs(p2[row, 2]) * Z) / Z + np.abs(g["uv"][..., row]) * U32
            per.append(du * SECOND + 2 * g["uv_err"][..., row])
        per = np.stack(per, -1).max(1)                       # [n,2]
        q = np.asarray(dets, np.float32).astype(np.float64)
        m = np.abs(np.asarray(lidar2cam, np.float64))
        loc_bound = 8 * U * (m[None, :3, 0] * np.abs(q[:, 0:1]) + m[None, :3, 1] * np.abs(q[:, 1:2]) + m[None, :3, 2] * np.abs(q[:, 2:3]) + m[None, :3, 3])
    return np.concatenate([per, per], 1), loc_bound
