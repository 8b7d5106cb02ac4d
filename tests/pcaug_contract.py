"""The three md_pc_* operators (include/minddet_hip_pcaug.h) restated in vectorised numpy float64, one sample at a time, with the margin
of every point-in-box and corner-in-range decision and with forward bounds of the reference's fp32 operation sequence.

Decisions.  A point is inside a box iff s = min(w/2 - |lx|, l/2 - |ly|, dz, h - dz) > 0; |s| is the distance to the nearest face, the
decision's margin.  A BEV corner is inside the range iff s = min(x - xmin, xmax - x, y - ymin, ymax - y) > 0.  A decision is DECIDED
when its margin exceeds MARGIN = 1e-4 m: the reference's fp32 sign expression (geometry.py:46-51) has products up to about 70 m x 8 m^2,
which is about 1e-5 m of error once divided by the normal's length; the margin is ten times that.  The collision decisions of
noise_per_object carry no margin here: the fixture's generator asserts that fp32 and float64 boxes select the same tries.

Bounds.  u = 2^-24.  The reference keeps boxes and points in fp32 and rounds after every step; a rotation x c + y s with c, s stored in
fp32 costs at most 4 u (|x| + |y|) and carries an earlier error e on as at most sqrt(2) e; an add or a scale costs u |result|.
point_bound / box_bound follow the reference's steps with these rules and add u |result| for the operator's own single rounding.
The v2 displacement (radius sin, radius cos of an fp32 atan2 minus the fp32 centre, preprocess.py:390-395, 417) is within
15 u radius: 3 u radius from the fp32 radius, 10 u radius from an angle that is off by at most 3 u pi, 2 u radius from the two stores.
"""
import numpy as np

MARGIN = 1e-4
U = 2.0 ** -24
NX = np.array([-0.5, -0.5, 0.5, 0.5])
NY = np.array([-0.5, 0.5, 0.5, -0.5])


def rect(w, l, ang):
    """corners of (w, l) rectangles rotated by ang about (0, 0): [..., 4] x, y (box2d_to_corner_jit's order and sense)"""
    c, s = np.cos(ang)[..., None], np.sin(ang)[..., None]
    px, py = NX * np.asarray(w)[..., None], NY * np.asarray(l)[..., None]
    return px * c + py * s, -px * s + py * c


def _covers(px, py, qx, qy):
    """every corner of Q strictly inside P; P, Q broadcastable [..., 4]"""
    ok = True
    for m in range(4):
        for k in range(4):
            k1 = (k + 1) % 4
            vx, vy = -(px[..., k] - px[..., k1]), -(py[..., k] - py[..., k1])
            cross = vy * (px[..., k] - qx[..., m]) - vx * (py[..., k] - qy[..., m])
            ok = ok & (cross < 0)
    return ok


def collide(ax, ay, bx, by):
    """box_collision_test's meaning (quirk (a)): (edges cross, A covers B, B covers A, collision); the first three are reported whatever
    the standup pre-test says, the last is gated by it"""
    iw = np.minimum(ax.max(-1), bx.max(-1)) - np.maximum(ax.min(-1), bx.min(-1))
    ih = np.minimum(ay.max(-1), by.max(-1)) - np.maximum(ay.min(-1), by.min(-1))
    cross = np.zeros(np.broadcast(ax[..., 0], bx[..., 0]).shape, bool)
    for k in range(4):
        for m in range(4):
            a0, a1, b0, b1 = ax[..., k], ay[..., k], ax[..., (k + 1) % 4], ay[..., (k + 1) % 4]
            c0, c1, d0, d1 = bx[..., m], by[..., m], bx[..., (m + 1) % 4], by[..., (m + 1) % 4]
            acd = (d1 - a1) * (c0 - a0) > (c1 - a1) * (d0 - a0)
            bcd = (d1 - b1) * (c0 - b0) > (c1 - b1) * (d0 - b0)
            abc = (c1 - a1) * (b0 - a0) > (b1 - a1) * (c0 - a0)
            abd = (d1 - a1) * (b0 - a0) > (b1 - a1) * (d0 - a0)
            cross |= (acd != bcd) & (abc != abd)
    a_b, b_a = _covers(ax, ay, bx, by), _covers(bx, by, ax, ay)
    return cross, a_b, b_a, (iw > 0) & (ih > 0) & (cross | a_b | b_a)


def noise_per_object(boxes, count, valid, loc, rot, grot=None):
    """one sample: boxes [G,7] f32, loc [G,T,3], rot [G,T], grot [G,T] or None -> selected [G] i32, obj_transform [G,4] f64,
    boxes_out [G,7] f32"""
    G, T = rot.shape
    b = boxes.astype(np.float64)
    sel = np.full(G, -1, np.int32)
    tf = np.zeros((G, 4))
    out = np.zeros((G, 7), np.float32)
    out[:count] = boxes[:count]
    tx, ty = rect(b[:count, 3], b[:count, 4], b[:count, 6])
    tx, ty = tx + b[:count, 0:1], ty + b[:count, 1:2]
    for i in range(count):
        if not valid[i]:
            continue
        x, y, w, l, r = b[i, 0], b[i, 1], b[i, 3], b[i, 4], b[i, 6]
        lx, ly, rn = loc[i, :, 0].copy(), loc[i, :, 1].copy(), rot[i].copy()
        px, py, ang = np.full(T, x), np.full(T, y), np.full(T, r)
        if grot is not None:
            # the centre turned about the origin by the try's angle (the reference: radius sin / cos of atan2(x, y) + g), formed
            # without the cancellation of two radius-sized terms: cos g - 1 = -2 sin^2(g / 2)
            g = grot[i]
            sg, cm1 = np.sin(g), -2.0 * np.sin(0.5 * g) ** 2
            dx, dy = x * cm1 + y * sg, y * cm1 - x * sg
            px, py, ang = x + dx, y + dy, r + g
            lx, ly, rn = lx + dx, ly + dy, rn + g
        rx, ry = rect(np.full(T, w), np.full(T, l), ang)
        c2, s2 = np.cos(rot[i])[:, None], np.sin(rot[i])[:, None]
        cx = (rx * c2 + ry * s2) + (px + loc[i, :, 0])[:, None]
        cy = (-rx * s2 + ry * c2) + (py + loc[i, :, 1])[:, None]
        hit = collide(cx[:, None, :], cy[:, None, :], tx[None], ty[None])[3]
        hit[:, i] = False
        clear = np.flatnonzero(~hit.any(1))
        if clear.size:
            j = int(clear[0])
            sel[i] = j
            tx[i], ty[i] = cx[j], cy[j]
            tf[i] = (lx[j], ly[j], loc[i, j, 2], rn[j])
            out[i, :3] = (b[i, :3] + tf[i, :3]).astype(np.float32)
            out[i, 6] = np.float32(b[i, 6] + tf[i, 3])
    return sel, tf, out


def signed_inside(points, boxes):
    """[N, K] signed distance to the nearest face, positive inside (float64)"""
    p, q = points.astype(np.float64), boxes.astype(np.float64)
    dx, dy, dz = (p[:, None, k] - q[None, :, k] for k in range(3))
    c, s = np.cos(q[:, 6])[None], np.sin(q[:, 6])[None]
    lx, ly = dx * c - dy * s, dx * s + dy * c
    return np.minimum(np.minimum(q[None, :, 3] / 2 - np.abs(lx), q[None, :, 4] / 2 - np.abs(ly)), np.minimum(dz, q[None, :, 5] - dz))


def _rot(x, y, ang):
    c, s = np.cos(ang), np.sin(ang)
    return x * c + y * s, -x * s + y * c


def augment_points(points, obj_boxes, count, valid, tf, glob, remove_boxes=None, remove_count=0, remove_from=0, box_err=None):
    """one sample -> dict: points (kept, in order) f32, owner [N] i32, decided [N] bool (every pair margin of the point above MARGIN),
    drop_decided (every remove-box pair decided: the kept count is then the reference's),
    near [N, K] bool (pairs within 1 m of a face), margin [N, K], bound [kept] (forward bound of the reference's fp32 sequence per
    kept point, max-norm over x, y, z; box_err [G]: what the owner's transform may differ by between reference and contract)"""
    N = len(points)
    act = np.flatnonzero(np.asarray(valid[:count]) != 0)
    s_obj = signed_inside(points, obj_boxes[:count][act]) if act.size else np.zeros((N, 0))
    owner = np.full(N, -1, np.int32)
    for k in range(act.size - 1, -1, -1):
        owner[s_obj[:, k] > 0] = act[k]
    margins = [np.abs(s_obj)]
    drop_decided = True
    if remove_boxes is not None and remove_count > 0:
        s_rem = signed_inside(points, remove_boxes[:remove_count])
        late = np.arange(N) >= remove_from
        owner[late & (s_rem > 0).any(1)] = -2
        margins.append(np.where(late[:, None], np.abs(s_rem), np.inf))
        drop_decided = bool((margins[-1] > MARGIN).all())
    margin = np.concatenate(margins, 1) if margins else np.zeros((N, 0))
    decided = (margin > MARGIN).all(1)
    keep = owner != -2
    p = points[keep].astype(np.float64)
    own = owner[keep]
    x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    e = np.zeros(len(p))
    m = (own >= 0) & (np.abs(tf[np.maximum(own, 0)]).sum(1) != 0)
    if m.any():
        t, c = tf[own[m]], obj_boxes[own[m]].astype(np.float64)
        dx, dy, dz = x[m] - c[:, 0], y[m] - c[:, 1], z[m] - c[:, 2]
        em = U * np.maximum(np.maximum(np.abs(dx), np.abs(dy)), np.abs(dz))
        rx, ry = _rot(dx, dy, t[:, 3])
        em = np.sqrt(2) * em + 4 * U * (np.abs(dx) + np.abs(dy))
        x1, y1, z1 = rx + c[:, 0], ry + c[:, 1], dz + c[:, 2]
        em += U * np.maximum(np.maximum(np.abs(x1), np.abs(y1)), np.abs(z1))
        x[m], y[m], z[m] = x1 + t[:, 0], y1 + t[:, 1], z1 + t[:, 2]
        em += U * np.maximum(np.maximum(np.abs(x[m]), np.abs(y[m])), np.abs(z[m]))
        if box_err is not None:
            em += box_err[own[m]]
        e[m] = em
    flip, ang, scale, t3 = glob[0] != 0, glob[1], glob[2], glob[3:6]
    if flip:
        y = -y
    e = np.sqrt(2) * e + 4 * U * (np.abs(x) + np.abs(y))
    x, y = _rot(x, y, ang)
    x, y, z = x * scale, y * scale, z * scale
    big = lambda: np.maximum(np.maximum(np.abs(x), np.abs(y)), np.abs(z))   # noqa: E731
    e = abs(scale) * e + U * big()
    x, y, z = x + t3[0], y + t3[1], z + t3[2]
    e += 2 * U * big()                                                      # the translation's rounding and the operator's own
    out = np.stack([x, y, z, p[:, 3]], 1).astype(np.float32) if len(p) else np.zeros((0, 4), np.float32)
    if len(p):
        out[:, 3] = points[keep][:, 3]
    near = margin < 1.0
    return dict(points=out, owner=owner, decided=decided, drop_decided=drop_decided, near=near, margin=margin, bound=e,
                exact=np.stack([x, y, z], 1))


def augment_boxes(boxes, count, valid, classes, glob, bv_range, in_err=None):
    """one sample -> dict: gt_boxes [G,7] f32 and gt_classes [G] i32 (compacted, zero rows behind), count, mask [count] (the range
    decision per input row, before `valid`), margin [count], all [count,7] f64 (every row transformed, the angle wrapped), bound
    [count,7] (forward bound per element; in_err [G,7]: error already in `boxes` against the reference's)"""
    G = len(boxes)
    b = boxes[:count].astype(np.float64)
    x, y, z, w, l, h, r = (b[:, k].copy() for k in range(7))
    e = np.zeros((count, 7)) if in_err is None else in_err[:count].copy()
    if glob[0] != 0:
        y, r = -y, -r + np.pi
        e[:, 6] += U * np.abs(r)
    exy = np.sqrt(2) * np.maximum(e[:, 0], e[:, 1]) + 4 * U * (np.abs(x) + np.abs(y))
    x, y = _rot(x, y, glob[1])
    r = r + glob[1]
    e[:, 0] = e[:, 1] = exy
    e[:, 6] += U * np.abs(r)
    s = glob[2]
    x, y, z, w, l, h = x * s, y * s, z * s, w * s, l * s, h * s
    e[:, :6] = abs(s) * e[:, :6] + U * np.abs(np.stack([x, y, z, w, l, h], 1))
    x, y, z = x + glob[3], y + glob[4], z + glob[5]
    e[:, :3] += U * np.abs(np.stack([x, y, z], 1))
    cx, cy = rect(w, l, r)
    cx, cy = cx + x[:, None], cy + y[:, None]
    sd = np.minimum(np.minimum(cx - bv_range[0], bv_range[2] - cx), np.minimum(cy - bv_range[1], bv_range[3] - cy))
    mask = (sd > 0).any(1)
    # the decision flips where the largest signed distance crosses zero
    margin = np.abs(sd.max(1)) if count else np.zeros(0)
    k = np.floor(r / (2 * np.pi) + 0.5)
    r = r - k * (2 * np.pi)
    e[:, 6] += 3 * U * 2 * np.pi * np.abs(k) + U * np.abs(r)
    allb = np.stack([x, y, z, w, l, h, r], 1) if count else np.zeros((0, 7))
    e += U * np.abs(allb)                                                   # the operator's own rounding
    keep = mask & (np.asarray(valid[:count]) != 0)
    out, cls = np.zeros((G, 7), np.float32), np.zeros(G, np.int32)
    n = int(keep.sum())
    out[:n], cls[:n] = allb[keep].astype(np.float32), np.asarray(classes[:count])[keep]
    return dict(gt_boxes=out, gt_classes=cls, count=n, mask=mask, margin=margin, all=allb, bound=e, keep=keep)


def transform_bound(boxes, count, sel, grot_used):
    """[G] bound on |loc x, y of the reference - contract| (0 without the global rotation: the draw itself is selected)"""
    b = boxes.astype(np.float64)
    radius = np.sqrt(b[:, 0] ** 2 + b[:, 1] ** 2)
    return np.where((np.arange(len(b)) < count) & (sel >= 0) & grot_used, 15 * U * radius, 0.0)
