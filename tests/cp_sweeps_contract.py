"""The contract of md_cp_sweeps_merge (include/minddet_hip_cpsweeps.h) in numpy float64: what tests/test_cp_sweeps_cpu.py holds against
the reference's own outputs (tests/golden/cp_sweeps_vectors.npz) and tests/test_cp_sweeps_gpu.py holds the kernels to.

Exact: the keep decision (an fp32 comparison of the untransformed values, both strict, NaN compares false), the order, column 3
(bit for bit), column 4 (fp32 of the time lag), the offsets, the status, the zero tail.
Values: a transformed coordinate is v = m0 x + m1 y + m2 z + m3, the explicit float64 sum from the left.  Any float64 evaluation of a
length-4 dot product (numpy's BLAS order, an FMA chain, the plain sum) lies within e = 4 * 2^-53 * (|m0 x| + |m1 y| + |m2 z| + |m3|)
of the exact value, the standard forward bound, so an output coordinate is right if it equals fp32(v) or lies between fp32(v - e)
and fp32(v + e).  The second branch matters only where v sits on an fp32 rounding boundary or the terms cancel; so that it cannot hide
a wrong kernel, at most FEW = 1 in 10^4 of a case's transformed coordinates may differ from fp32(v) (the cap of the other *aug tests).
An untransformed coordinate is the input's bits."""
import numpy as np

U = 2.0 ** -53
FEW = 1e-4
REMOVE_CLOSE, TRANSFORM = 1, 2


def keep_mask(rows, radius):
    """remove_close on fp32 rows [n, >= 2]: True = kept"""
    r = np.float32(radius)
    with np.errstate(invalid="ignore"):
        return ~((np.abs(rows[:, 0]) < r) & (np.abs(rows[:, 1]) < r))


def transform(m12, xyz):
    """m12: 12 float64 (rows 0-2 of the 4x4), xyz [n,3] fp32 -> (v [n,3] float64, e [n,3] float64)"""
    m = np.asarray(m12, np.float64).reshape(3, 4)
    x, y, z = (xyz[:, k].astype(np.float64) for k in range(3))
    v, e = np.empty((len(xyz), 3)), np.empty((len(xyz), 3))
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            t0, t1, t2 = m[r, 0] * x, m[r, 1] * y, m[r, 2] * z
            v[:, r] = ((t0 + t1) + t2) + m[r, 3]
            e[:, r] = 4 * U * (np.abs(t0) + np.abs(t1) + np.abs(t2) + abs(m[r, 3]))
    return v, e


def merge(points, seg_range, transforms, time_lag, seg_flags, radius, M=None):
    """the operator on host arrays -> dict(points [M,5] fp32 with fp32(v) in the transformed coordinates, offsets [B+1] i32,
    status [B] i32, lo / hi [n,3] fp32: the interval of every coordinate of the n kept rows (lo == hi == the value where it is
    exact), transformed [n] bool, src [n]: the row of `points` each kept row came from)"""
    points = np.asarray(points, np.float32)
    N = len(points)
    M = N if M is None else M
    seg_range, seg_flags = np.asarray(seg_range, np.int64), np.asarray(seg_flags, np.int64)
    B, S = seg_range.shape[:2]
    in_range = ((seg_range >= 0) & (seg_range <= N)).all(2)
    lens = np.where(in_range, np.maximum(seg_range[..., 1] - seg_range[..., 0], 0), 0)
    over = int(lens.sum()) > N
    status = (~in_range.all(1)).astype(np.int32) | (2 if over else 0)
    rows, lo, hi, tf_mask, src, offsets = [], [], [], [], [], [0]
    for b in range(B):
        for s in range(S if status[b] == 0 else 0):
            b0, e0 = (int(v) for v in seg_range[b, s])
            if e0 <= b0:
                continue
            idx = np.arange(b0, e0)
            seg = points[idx, :4]
            if seg_flags[b, s] & REMOVE_CLOSE:
                k = keep_mask(seg, radius)
                idx, seg = idx[k], seg[k]
            out = np.zeros((len(seg), 5), np.float32)
            out[:, :4] = seg
            out[:, 4] = np.float32(np.float64(time_lag[b, s]))
            l, h = seg[:, :3].copy(), seg[:, :3].copy()
            if seg_flags[b, s] & TRANSFORM:
                v, e = transform(transforms[b, s], seg[:, :3])
                with np.errstate(invalid="ignore", over="ignore"):
                    out[:, :3] = v.astype(np.float32)
                    l, h = (v - e).astype(np.float32), (v + e).astype(np.float32)
            rows.append(out); lo.append(l); hi.append(h); src.append(idx)
            tf_mask.append(np.full(len(seg), bool(seg_flags[b, s] & TRANSFORM)))
        offsets.append(sum(len(r) for r in rows))
    n = offsets[-1]
    full = np.zeros((M, 5), np.float32)
    if n:
        full[:n] = np.concatenate(rows)
    cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dt)      # noqa: E731
    return dict(points=full, offsets=np.asarray(offsets, np.int32), status=status, lo=cat(lo, (0, 3), np.float32), hi=cat(hi, (0, 3), np.float32),
                transformed=cat(tf_mask, (0,), bool), src=cat(src, (0,), np.int64))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check(got_points, got_offsets, c, what=""):
    """holds an output (points [M,5], offsets) to the contract dict c of merge(): the exact parts exact, xyz within the condition and
    the cap.  -> (transformed coordinates that differ from fp32(v), their number)"""
    got_points, want = np.asarray(got_points, np.float32), c["points"]
    assert np.array_equal(np.asarray(got_offsets), c["offsets"]), (what, np.asarray(got_offsets).tolist(), c["offsets"].tolist())
    n = int(c["offsets"][-1])
    assert got_points.shape == want.shape and same_bits(got_points[n:], want[n:]), (what, "the zero tail")
    assert same_bits(got_points[:n, 3:], want[:n, 3:]), (what, "columns 3 and 4")
    t = c["transformed"]
    assert same_bits(got_points[:n][~t, :3], want[:n][~t, :3]), (what, "untransformed xyz")
    g, w = got_points[:n][t, :3], want[:n][t, :3]
    same = (g.view(np.uint32) == w.view(np.uint32)) | (g == w)
    with np.errstate(invalid="ignore"):
        inside = (g >= c["lo"][t]) & (g <= c["hi"][t])
    both_nan = np.isnan(g) & np.isnan(w)
    ok = same | inside | both_nan
    differ = int((~(same | both_nan)).sum())
    print(f"{what}: {differ} of {g.size} transformed coordinates differ from fp32(v), {int((~ok).sum())} outside the interval")
    assert ok.all(), (what, int((~ok).sum()))
    assert differ <= FEW * g.size, (what, differ, g.size)
    return differ, g.size
