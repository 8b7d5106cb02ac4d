"""Float64 contract of the NMS family (csrc/nms.hip): judges, error bands, seeded list generators.  numpy, CPU only.

The device tests of tests/test_nms_iou_gpu.py compare the kernels with oracle/det_oracle.c, an fp32 restatement of the same
arithmetic: bit-exactness is pinned there, a misreading shared by kernel and oracle is not.  This module states what a greedy NMS
keep list has to satisfy in terms of the GEOMETRY of the boxes, evaluated in float64, and validates a keep list against it
(`judge_greedy`); it never reproduces the kernel's fp32 decisions.

Operators (a pair = an earlier KEPT box of the same group against a later box; t = float64(float32(thr))):
    md_nms_aligned mode 0        suppress iff ovr >= t     ovr = inter / (sa + sb - inter), eps on every width / height
    md_nms_aligned mode 1        suppress iff ovr >  t     the same with +1 pixel instead of eps
    md_nms_aligned mode 2        suppress iff ovr >  t     ovr = inter / fmaxf(sa + sb - inter, 1e-8)
    NmsNormalGpu                 suppress iff iou >  t     footprint (x -+ dx/2, y -+ dy/2), fmaxf(union, 1e-8)
    NmsGpu                       suppress iff iou >  t     rotated overlap / fmaxf(sa + sb - overlap, 1e-8)
    boxes_iou_nms_gpu            suppress iff ovr >= t     rotated overlap / (sa + sb - overlap); dead rule below
    md_circle_nms                suppress iff d2  <= t     d2 = squared centre distance
NaN rule: an IoU of NaN compares false in both directions.  A pair whose quantity is NaN neither suppresses nor is suppressed,
under every operator above (also under `<=`), so a box whose every pair is NaN is kept.  Which quantity a NaN coordinate gives
differs per op:
    md_nms_aligned modes 0, 1, boxes_iou_nms_gpu, md_circle_nms   unclamped: the quantity is NaN, the box is kept and drops nothing
    md_nms_aligned mode 2     fmaxf(NaN union, 1e-8) = 1e-8 and the ternary min / max keep or drop a NaN edge by operand order:
                              the ovr is inter / 1e-8 or 0, so a partly NaN box can suppress (NaN x1 / y1) and be suppressed
                              (NaN x2 / y2); an all-NaN box has inter 0, ovr 0
    NmsNormalGpu              fmaxf / fminf drop a NaN edge: along an axis with a NaN centre or size the box takes the other box's
                              extent; a NaN dx or dy also makes the union NaN, which clamps to 1e-8: iou = inter / 1e-8.  Such a
                              box suppresses and is suppressed by what its remaining extent overlaps
    NmsGpu                    every comparison of the clipping is false: overlap 0, iou 0 / 1e-8 = 0, kept and drops nothing
aligned_ovr and normal_iou evaluate the kernels' own min / max forms, so the bands follow these rules.
Dead rule (boxes_iou_nms_gpu only): a box with dx * dy == 0 in fp32 is never kept and never suppresses.
Count clamp: a list's length is min(count, N) (count NULL = N); boxes at or after it are never kept and never suppress.
Quota: with max_output = q > 0 the list is cut after the q-th kept box.

Bands.  `pair_band(i, js)` returns float64 (lo, hi) with lo <= kernel's fp32 quantity <= hi for box i against each earlier box of
js.  A pair SURELY suppresses when the whole band is on the suppressing side of t, it MAY suppress when any of it is; a pair with
t strictly inside the band is undecided and only weakens the check (it is never left out).  u = 2^-24 below.

  aligned (modes 0/1/2): v = the mode's formula in float64 on the fp32 coordinates, band v -+ 32 u |v|.  Each edge length takes
    two roundings (the difference, the + off): (1+u)^2.  inter = w * h: 2 + 2 + 1 = 5 u.  Each area likewise 5 u.  The union
    sa + sb - inter adds two roundings and cancels: its absolute error is at most 5 u (sa + sb + inter) + 2 u (sa + sb), and
    sa + sb + inter <= 3 union, so at most 19 u relative.  One rounding on the quotient: 5 + 19 + 1 = 25 u, rounded up to 32 u.
    The float64 formula keeps the kernel's ternary min / max and fmaxf, so a NaN or infinite coordinate gives the same class of
    result (NaN, 0 or inf) as in fp32.
  circle: d2 in float64, band -+ 8 u d2 (dx, dy one rounding each, squared: 2 u + 1 u each, one for the sum: under 6 u).
  normal (NmsNormalGpu): the edges are c -+ d/2, one rounding each of absolute size u E with E = |c| + d/2: the error is absolute
    in the coordinate magnitude, not relative in the overlap.  Running bound per pair, with Ex, Ey the largest edge magnitude of
    the pair per axis, w, h, I, U, v the float64 width, height, intersection, union and IoU:
        dw = u (2 Ex + w)         dh = u (2 Ey + h)                 (two edges, one subtraction; fmaxf(., 0) is 1-Lipschitz)
        dI = w dh + h dw + dw dh + u I
        dU = dI + 3 u (sa + sb) + 2 u U                             (two areas one rounding each, two additions)
        dv = (dI + v dU) / (U - dU) + u v                           (U - dU <= 0: the pair is undecided)
    and the band is v -+ 1.01 dv (1 % for the second-order terms).
  rotated (NmsGpu, boxes_iou_nms_gpu, BoxesIouBevGpu, BoxesOverlapBevGpu): pure geometry, independent of how the kernel clips.
    The kernel's polygon has as vertices the crossings of the true edges, the corners of B within MARGIN = 0.01 of A and the
    corners of A within MARGIN of B.  All of them lie in the rectangles grown by MARGIN (both convex), and the vertices of the true
    intersection are among them, so
        lo = float64 convex-clip area of the two rectangles,  hi = the same with every half-extent enlarged by MARGIN,
    and when both rectangles are single points (dx = dy = 0 twice) every vertex is one of the two points and the area is 0.
    Exactly parallel, collinear edges are outside this argument (the reference's crossing test is strict and its fp32 cross
    products then decide by rounding): the generators jitter yaw and size, and rot_nested_ties, the one yaw-0 list, shares no edge
    line between its boxes.
    The fp32 evaluation (trig rounded once, crossings, angular sort, fan area) adds a measured slack: over every rotated generator
    of this file (rot_lists(): 16 lists) the largest excursion of oracle.boxes_overlap_bev outside
    [lo, hi], relative to 1 + hi, was ROT_SLACK_MEASURED = 4.92e-5 (a sliver of 0.0013 m2 between second neighbours of a chain;
    7.1e-6 on the clustered lists; tests/test_nms_contract_cpu.py re-measures it), and the band uses ROT_SLACK = 4 x that =
    1.97e-4.  Overlap band [max(lo - s, 0), hi + s], s = ROT_SLACK (1 + hi) where hi > 0.  It becomes an IoU band through the
    op's denominator rule (monotone in the overlap), widened by 16 u relative for the fp32 areas, the union's two roundings with
    cancellation (<= 3x) and the quotient.  Zero-area boxes under NmsGpu have IoU = overlap / 1e-8 with an overlap anywhere in
    [0, 4e-4]: the geometry leaves those pairs undecided by construction (rot_dead_only).

Lattice regime.  Aligned boxes with integer coordinates below 2^11 and eps 0 or mode 1, circle centres on integers: every fp32
operation is exact and the quotient of two integers below 2^24 is rounded once, which float32(float64 quotient) reproduces (53 >=
2 * 24 + 2: no double rounding).  `exact=True` bands have zero width there, the judge then admits exactly one keep list, and
`greedy_exact` computes it.
"""
import numpy as np

U = 2.0 ** -24
MARGIN = float(np.float32(1e-2))
EPS8 = float(np.float32(1e-8))
TILE = 64
SCAN_KEEP_CAP = 4096
# largest excursion of the fp32 oracle's rotated overlap outside the geometric band, relative to 1 + hi, over rot_lists()
# (measured by test_rotated_slack_is_the_measured_one_times_four), and the slack the bands use
ROT_SLACK_MEASURED = 4.92e-5
ROT_SLACK = 4 * ROT_SLACK_MEASURED


class ContractViolation(AssertionError):
    pass


def thr64(thr):
    return float(np.float32(thr))


# ------------------------------------------------------------------------------------------------ operators and the judge
def surely(op, lo, hi, t):
    if op == "ge":
        return lo >= t
    if op == "gt":
        return lo > t
    assert op == "le"
    return hi <= t


def maybe(op, lo, hi, t):
    if op == "ge":
        return hi >= t
    if op == "gt":
        return hi > t
    assert op == "le"
    return lo <= t


def keep_from_outputs(n_max, num, keep_idx, keep_mask=None):
    """num / keep_idx / keep_mask of one list agree; returns the keep list.  keep_idx: leading num valid, the rest 0."""
    num = int(num)
    keep_idx = np.asarray(keep_idx).astype(np.int64)
    if not (0 <= num <= n_max and keep_idx.shape[0] >= n_max):
        raise ContractViolation(f"num {num} outside [0, {n_max}]")
    if (keep_idx[num:] != 0).any():
        raise ContractViolation("tail of keep_idx is not 0")
    keep = keep_idx[:num]
    if ((keep < 0) | (keep >= n_max)).any():
        raise ContractViolation("kept index outside the list")
    if keep_mask is not None:
        want = np.zeros(n_max, np.uint8)
        want[keep] = 1
        if not np.array_equal(np.asarray(keep_mask)[:n_max], want) or int(want.sum()) != num:
            raise ContractViolation("keep_mask, keep_idx and num disagree")
    return keep


def judge_greedy(pair_band, n, keep, groups=None, dead=None, quota=0, *, op, thr):
    """Validate a greedy-NMS keep list of the first n boxes of a list; returns (undecided pairs, judged pairs).

    Valid iff: indices ascend and are < n; no kept box is dead or surely suppressed by an earlier kept box of its group; every
    dropped box up to the quota point is dead or has an earlier kept box of its group that may suppress it; at most `quota` boxes
    are kept (quota > 0) and nothing after the quota-th."""
    t = thr64(thr)
    keep = np.asarray(keep).astype(np.int64)
    if keep.size and ((np.diff(keep) <= 0).any() or keep[0] < 0 or keep[-1] >= n):
        raise ContractViolation("kept indices do not ascend inside [0, n)")
    if quota > 0 and keep.size > quota:
        raise ContractViolation(f"{keep.size} kept with a quota of {quota}")
    limit = int(keep[-1]) + 1 if (quota > 0 and keep.size == quota) else n
    kept = np.zeros(n, bool)
    kept[keep] = True
    undecided = judged = 0
    for j in range(limit):
        ks = keep[: np.searchsorted(keep, j)]
        if groups is not None:
            ks = ks[groups[ks] == groups[j]]
        if dead is not None and dead[j]:
            if kept[j]:
                raise ContractViolation(f"dead box {j} kept")
            continue
        if ks.size:
            lo, hi = pair_band(j, ks)
            sure, may = surely(op, lo, hi, t), maybe(op, lo, hi, t)
            judged += ks.size
            undecided += int((may & ~sure).sum())
        else:
            sure = may = np.zeros(0, bool)
        if kept[j]:
            if sure.any():
                raise ContractViolation(f"box {j} kept although box {int(ks[np.argmax(sure)])} surely suppresses it")
        elif not may.any():
            raise ContractViolation(f"box {j} dropped although no earlier kept box of its group can suppress it")
    return undecided, judged


def greedy_exact(pair_band, n, groups=None, dead=None, quota=0, *, op, thr):
    """The one valid keep list under a zero-width band (lattice regime)."""
    t = thr64(thr)
    keep = []
    for j in range(n):
        if quota > 0 and len(keep) >= quota:
            break
        if dead is not None and dead[j]:
            continue
        ks = np.asarray(keep, np.int64)
        if groups is not None and ks.size:
            ks = ks[groups[ks] == groups[j]]
        if ks.size:
            lo, hi = pair_band(j, ks)
            assert np.array_equal(lo, hi, equal_nan=True), "greedy_exact needs an exact band"
            if surely(op, lo, hi, t).any():
                continue
        keep.append(j)
    return np.asarray(keep, np.int64)


# ------------------------------------------------------------------------------------------------ the quantities, any dtype
def _lo(a, b):
    return np.where(a > b, b, a)   # the kernels' ternary min / max (rlo / rhi), NaN behaviour included


def _hi(a, b):
    return np.where(a > b, a, b)


def aligned_ovr(rows, col, off, mode, dt=np.float64):
    """md_nms_aligned's quantity for kept row boxes [m,4] against one column box [4], evaluated in dtype dt."""
    a, c = np.asarray(rows, dt), np.asarray(col, dt)
    off, zero = dt(off), dt(0)
    with np.errstate(all="ignore"):
        area_a = (a[:, 2] - a[:, 0] + off) * (a[:, 3] - a[:, 1] + off)
        area_c = (c[2] - c[0] + off) * (c[3] - c[1] + off)
        w = _hi(_lo(a[:, 2], c[2]) - _hi(a[:, 0], c[0]) + off, zero)
        h = _hi(_lo(a[:, 3], c[3]) - _hi(a[:, 1], c[1]) + off, zero)
        inter = w * h
        union = area_a + area_c - inter
        if mode == 2:
            union = np.fmax(union, dt(np.float32(1e-8)))
        return (inter / union).astype(dt)


def normal_iou(rows, col, dt=np.float64):
    """NmsNormalGpu's quantity (iou_normal of the x, y, dx, dy footprint of 7-float boxes)."""
    a, b = np.asarray(rows, dt), np.asarray(col, dt)
    two = dt(2)
    with np.errstate(all="ignore"):
        left = np.fmax(a[:, 0] - a[:, 3] / two, b[0] - b[3] / two)
        right = np.fmin(a[:, 0] + a[:, 3] / two, b[0] + b[3] / two)
        top = np.fmax(a[:, 1] - a[:, 4] / two, b[1] - b[4] / two)
        bottom = np.fmin(a[:, 1] + a[:, 4] / two, b[1] + b[4] / two)
        w, h = np.fmax(right - left, dt(0)), np.fmax(bottom - top, dt(0))
        inter = w * h
        return (inter / np.fmax(a[:, 3] * a[:, 4] + b[3] * b[4] - inter, dt(np.float32(1e-8)))).astype(dt)


def circle_d2(rows, col, dt=np.float64):
    a, c = np.asarray(rows, dt), np.asarray(col, dt)
    dx, dy = a[:, 0] - c[0], a[:, 1] - c[1]
    return dx * dx + dy * dy


def _is_lattice(x):
    x = np.asarray(x, np.float64)
    return bool(np.isfinite(x).all() and (x == np.round(x)).all() and (np.abs(x) < 2 ** 11).all())


# ------------------------------------------------------------------------------------------------ bands
def aligned_band(boxes, mode, eps=0.0, exact=False):
    b = np.asarray(boxes, np.float32).astype(np.float64)
    off = 1.0 if mode == 1 else float(np.float32(eps))
    if exact:
        assert _is_lattice(b) and off in (0.0, 1.0), "exact band outside the lattice regime"

    def band(i, js):
        v = aligned_ovr(b[js], b[i], off, mode)
        if exact:
            v = v.astype(np.float32).astype(np.float64)   # the once-rounded quotient of two integers below 2^24
            return v, v
        d = np.where(np.isinf(v), 0.0, 32 * U * np.abs(v))       # an infinite ovr (inf / 1e-8) is infinite in fp32 too
        return v - d, v + d
    return band


def circle_band(xy, exact=False):
    p = np.asarray(xy, np.float32).astype(np.float64)
    if exact:
        assert _is_lattice(p)

    def band(i, js):
        v = circle_d2(p[js], p[i])
        d = 0.0 if exact else 8 * U * v
        return v - d, v + d
    return band


def normal_band(boxes):
    b = np.asarray(boxes, np.float32).astype(np.float64)
    ex = np.abs(b[:, 0]) + b[:, 3] / 2
    ey = np.abs(b[:, 1]) + b[:, 4] / 2
    area = b[:, 3] * b[:, 4]

    def band(i, js):
        a, c = b[js], b[i]
        w = np.maximum(np.minimum(a[:, 0] + a[:, 3] / 2, c[0] + c[3] / 2) - np.maximum(a[:, 0] - a[:, 3] / 2, c[0] - c[3] / 2), 0)
        h = np.maximum(np.minimum(a[:, 1] + a[:, 4] / 2, c[1] + c[4] / 2) - np.maximum(a[:, 1] - a[:, 4] / 2, c[1] - c[4] / 2), 0)
        inter = w * h
        s = area[js] + area[i]
        un = np.maximum(s - inter, EPS8)
        v = inter / un
        dw = U * (2 * np.maximum(ex[js], ex[i]) + w)
        dh = U * (2 * np.maximum(ey[js], ey[i]) + h)
        di = w * dh + h * dw + dw * dh + U * inter
        du = di + 3 * U * s + 2 * U * un
        den = un - du
        with np.errstate(all="ignore"):
            dv = np.where(den > 0, 1.01 * ((di + v * du) / den + U * v), np.inf)
        lo, hi = v - dv, v + dv
        odd = ~(np.isfinite(a[:, [0, 1, 3, 4]]).all(1) & np.isfinite(c[[0, 1, 3, 4]]).all())
        if odd.any():
            # a NaN or infinite x, y, dx, dy: fmaxf / fminf drop a NaN edge and fmaxf(NaN union, 1e-8) is 1e-8, so the kernel's
            # IoU is that of the remaining extent, over 1e-8 where the union is NaN; the running bound does not apply: 0.1 %
            # around the kernel's formula in float64, and undecided where a remaining extent is within 1e-3 of zero
            vo = normal_iou(a[odd], c)
            with np.errstate(all="ignore"):
                wr = np.fmin(a[odd, 0] + a[odd, 3] / 2, c[0] + c[3] / 2) - np.fmax(a[odd, 0] - a[odd, 3] / 2, c[0] - c[3] / 2)
                hr = np.fmin(a[odd, 1] + a[odd, 4] / 2, c[1] + c[4] / 2) - np.fmax(a[odd, 1] - a[odd, 4] / 2, c[1] - c[4] / 2)
            graze = (np.abs(wr) < 1e-3) | (np.abs(hr) < 1e-3)
            lo[odd] = np.where(graze, 0.0, vo * (1 - 1e-3))
            hi[odd] = np.where(graze, np.inf, vo * (1 + 1e-3))
        return lo, hi
    return band


def rect_corners(b, margin=0.0):
    """[m,7] boxes -> [m,4,2] float64 corners, counter-clockwise, half-extents enlarged by `margin`."""
    b = np.asarray(b, np.float64)
    hx, hy = b[:, 3] / 2 + margin, b[:, 4] / 2 + margin
    c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
    px = np.stack([-hx, hx, hx, -hx], 1)
    py = np.stack([-hy, -hy, hy, hy], 1)
    return np.stack([px * c[:, None] - py * s[:, None] + b[:, 0:1], px * s[:, None] + py * c[:, None] + b[:, 1:2]], -1)


def clip_area(A, B):
    """Area of the intersection of convex counter-clockwise quadrilaterals A[m,4,2] and B[m,4,2] (Sutherland-Hodgman in float64,
    vectorised over m; a spare slot repeats the last vertex, which leaves the shoelace sum unchanged)."""
    poly = np.array(A, np.float64)
    m = poly.shape[0]
    empty = np.zeros(m, bool)
    for e in range(4):
        p0, p1 = B[:, e], B[:, (e + 1) % 4]
        ex, ey = (p1 - p0)[:, 0:1], (p1 - p0)[:, 1:2]
        d = ex * (poly[..., 1] - p0[:, 1:2]) - ey * (poly[..., 0] - p0[:, 0:1])
        dn, pn = np.roll(d, -1, 1), np.roll(poly, -1, 1)
        ins, ins_n = d >= 0, dn >= 0
        cross = ins != ins_n
        with np.errstate(all="ignore"):
            t = np.where(cross, d / np.where(cross, d - dn, 1.0), 0.0)
        X = poly + t[..., None] * (pn - poly)
        K = poly.shape[1]
        out = np.empty((m, 2 * K, 2))
        out[:, 0::2], out[:, 1::2] = X, pn
        valid = np.empty((m, 2 * K), bool)
        valid[:, 0::2], valid[:, 1::2] = cross, ins_n
        # a convex polygon gains at most one vertex per clip: the valid slots, in order, into K + 1 slots, the last one repeated
        order = np.argsort(~valid, axis=1, kind="stable")[:, : K + 1]
        cnt = valid.sum(1)
        q = np.minimum(np.arange(K + 1)[None, :], np.maximum(cnt, 1)[:, None] - 1)
        idx = np.take_along_axis(order, q, 1)
        empty |= cnt == 0
        poly = np.take_along_axis(out, idx[..., None], 1)
    x, y = poly[..., 0], poly[..., 1]
    area = 0.5 * np.abs((x * np.roll(y, -1, 1) - np.roll(x, -1, 1) * y).sum(1))
    return np.where(empty, 0.0, area)


def rot_overlap_band(rows, col):
    """Geometry-only (lo, hi) of the rotated overlap area of row boxes [m,7] against column boxes [m,7] (or one [7])."""
    a = np.asarray(rows, np.float32).astype(np.float64)
    c = np.broadcast_to(np.asarray(col, np.float32).astype(np.float64), a.shape)
    flat = (a[:, 3] * a[:, 4] == 0) | (c[:, 3] * c[:, 4] == 0)     # a segment or a point has no interior to clip against
    lo = np.where(flat, 0.0, clip_area(rect_corners(a), rect_corners(c)))
    hi = np.maximum(clip_area(rect_corners(a, MARGIN), rect_corners(c, MARGIN)), lo)
    points = (a[:, 3] == 0) & (a[:, 4] == 0) & (c[:, 3] == 0) & (c[:, 4] == 0)
    hi = np.where(points, 0.0, hi)
    return lo, hi


def with_rot_slack(lo, hi):
    """Geometry-only overlap band -> the band with the measured fp32 slack (none where the geometry says exactly 0 for two points)."""
    s = np.where(hi > 0, ROT_SLACK * (1 + hi), 0.0)
    return np.maximum(lo - s, 0.0), hi + s


def rot_iou_from_overlap(lo, hi, sa, sb, rule):
    """Overlap band -> IoU band under the op's denominator rule: 'clamp' = / fmaxf(sa+sb-o, 1e-8), 'none' = / (sa+sb-o)."""
    s = sa + sb
    with np.errstate(all="ignore"):
        if rule == "clamp":
            vlo, vhi = lo / np.maximum(s - lo, EPS8), hi / np.maximum(s - hi, EPS8)
        else:
            vlo = lo / (s - lo)                                  # 0/0 = NaN: compares false
            vhi = np.where(s - hi > 0, hi / (s - hi), np.where(np.isnan(vlo), np.nan, np.inf))
    return vlo * (1 - 16 * U), vhi * (1 + 16 * U)


def rot_overlap_matrix(a, b):
    """Geometry-only (lo, hi)[na, nb] of the rotated overlap of every box of a against every box of b."""
    a, b = np.asarray(a), np.asarray(b)
    if a is b or (a.shape == b.shape and np.array_equal(a, b, equal_nan=True)):     # the band is symmetric: one triangle
        iu, ju = np.triu_indices(len(a))
        lo, hi = np.zeros((len(a), len(a))), np.zeros((len(a), len(a)))
        lo[iu, ju], hi[iu, ju] = rot_overlap_band(a[iu], a[ju])
        lo[ju, iu], hi[ju, iu] = lo[iu, ju], hi[iu, ju]
        return lo, hi
    ii, jj = np.meshgrid(np.arange(len(a)), np.arange(len(b)), indexing="ij")
    lo, hi = rot_overlap_band(a[ii.ravel()], b[jj.ravel()])
    return lo.reshape(len(a), len(b)), hi.reshape(len(a), len(b))


def rot_band(boxes, rule, ov=None):
    """ov: the geometry-only rot_overlap_matrix(boxes, boxes), to share it between the two rules and several judgements of a list."""
    b = np.asarray(boxes, np.float32).astype(np.float64)
    area = b[:, 3] * b[:, 4]
    lo, hi = with_rot_slack(*(rot_overlap_matrix(b, b) if ov is None else ov))

    def band(i, js):
        return rot_iou_from_overlap(lo[js, i], hi[js, i], area[js], area[i], rule)
    return band


def rot_dead(boxes):
    b = np.asarray(boxes, np.float32)
    return (b[:, 3] * b[:, 4]) == 0


# ------------------------------------------------------------------------------------------------ generators (all seeded)
def clustered_aligned(n, nobj, seed, ngroups=1, W=1344.0, H=800.0):
    """n corner boxes around nobj objects: position jitter 6 % of the size, size jitter 12 %; class key per object."""
    rng = np.random.default_rng(seed)
    cx, cy = rng.uniform(0, W, nobj), rng.uniform(0, H, nobj)
    w = np.exp(rng.uniform(np.log(24), np.log(300), nobj))
    h = np.exp(rng.uniform(np.log(24), np.log(300), nobj))
    cls = rng.integers(0, ngroups, nobj)
    o = rng.integers(0, nobj, n)
    bx = cx[o] + rng.normal(0, 0.06, n) * w[o]
    by = cy[o] + rng.normal(0, 0.06, n) * h[o]
    bw, bh = w[o] * np.exp(rng.normal(0, 0.12, n)), h[o] * np.exp(rng.normal(0, 0.12, n))
    boxes = np.stack([bx - bw / 2, by - bh / 2, bx + bw / 2, by + bh / 2], 1).astype(np.float32)
    return boxes, cls[o].astype(np.int32)


def chain_step(size, thr):
    """Shift s of equal boxes of extent `size` along one axis with IoU(s) = (size-s)/(size+s) > thr > IoU(2s)."""
    top = size * (1 - thr) / (1 + thr)     # IoU(top) = thr ; IoU(2 * top/2) = thr
    return 0.75 * top


def chain_aligned(n, thr, seed, size=200.0, lead=1):
    """`lead` far-away boxes, then a chain along x: neighbours suppress, second neighbours do not (at thr, every mode).  With
    lead = 1 the kept boxes are the odd indices, so each 64-box tile boundary has a kept box at 64k-1 suppressing box 64k."""
    rng = np.random.default_rng(seed)
    s = chain_step(size, thr)
    x = np.arange(n - lead) * s
    y = rng.uniform(0, 2.0, n - lead)
    b = np.stack([x, y, x + size, y + 120.0], 1)
    far = np.stack([np.arange(lead) * 400.0, np.full(lead, 5000.0), np.arange(lead) * 400.0 + 100, np.full(lead, 5100.0)], 1)
    return np.concatenate([far, b]).astype(np.float32)


def slot_aligned(pattern, seed, cell=40, per_row=48, jitter=1.0):
    """Box k sits in cell pattern[k] of a grid of disjoint cells; boxes of one cell overlap with IoU > 0.8, so the first box of
    every cell is kept and every later one dropped, at every threshold used."""
    rng = np.random.default_rng(seed)
    p = np.asarray(pattern)
    ox, oy = (p % per_row) * cell, (p // per_row) * cell
    j = rng.uniform(-jitter / 2, jitter / 2, (len(p), 4))
    return (np.stack([ox + 4, oy + 4, ox + 36, oy + 36], 1) + j).astype(np.float32)


def lattice_ties(mode, thr):
    """Integer boxes with pairs of IoU exactly thr (1/2 or 1/4), some plain pairs, one pair per 40-pixel row."""
    k = {0.5: 2, 0.25: 4}[thr]
    p = 1 if mode == 1 else 0          # +1 pixel: a width of w pixels is x2 - x1 = w - 1
    rows = []
    for r, (a, b) in enumerate([(10, 7), (16, 20), (3, 30), (25, 25)]):
        y = 40 * r
        rows += [[0, y, k * a - p, y + b - p], [0, y, a - p, y + b - p]]            # IoU exactly 1/k
        rows += [[300, y, 300 + k * a - p, y + b - p], [300, y, 300 + a + 1 - p, y + b - p]]   # just above 1/k
        rows += [[600, y, 600 + k * a + 1 - p, y + b - p], [600, y, 600 + a - p, y + b - p]]   # just below 1/k
    return np.asarray(rows, np.float32)


def lattice_clustered(n, seed, mode):
    """Integer boxes below 2^11 around a few objects, with the exact-tie pairs of lattice_ties spliced in at thr 0.5 and 0.25."""
    rng = np.random.default_rng(seed)
    nobj = max(2, n // 24)
    cx, cy = rng.integers(200, 1800, nobj), rng.integers(400, 1800, nobj)
    w, h = rng.integers(20, 120, nobj), rng.integers(20, 120, nobj)
    o = rng.integers(0, nobj, n)
    x1 = cx[o] + rng.integers(-4, 5, n)
    y1 = cy[o] + rng.integers(-4, 5, n)
    b = np.stack([x1, y1, x1 + w[o] + rng.integers(-6, 7, n), y1 + h[o] + rng.integers(-6, 7, n)], 1).astype(np.float32)
    ties = np.concatenate([lattice_ties(mode, 0.5), lattice_ties(mode, 0.25) + np.float32([0, 200, 0, 200])])
    m = min(len(ties), n) // 2 * 2
    # a tie pair keeps its order (the larger box first) but lands at random ranks, other pairs and tile boundaries in between
    at = np.sort(rng.choice(n, m, replace=False))
    b[at[0::2]], b[at[1::2]] = ties[0:m:2], ties[1:m:2]
    assert _is_lattice(b)
    return b


def nan_inf_aligned(n, seed):
    """A clustered list with an all-NaN box (at n // 3), a box of infinite width (n // 2) and, from 20 boxes on, boxes with one NaN
    coordinate: x1 (n // 4), x2 (2 n // 3), y1 (n // 5), y2 (3 n // 4).  Modes 0 and 1 give every pair of such a box NaN, which
    compares false.  Mode 2 clamps a NaN union to 1e-8: a box with NaN x1 or y1 suppresses what it overlaps, a box with NaN x2 or
    y2 is suppressed by what overlaps it; aligned_ovr models both."""
    b, g = clustered_aligned(n, 6, seed)
    if n >= 20:
        b[n // 4, 0] = b[2 * n // 3, 2] = b[n // 5, 1] = b[3 * n // 4, 3] = np.nan
    b[n // 3] = np.nan
    b[n // 2, 2] = np.inf
    return b, g


def nan_normal(n, seed):
    """Clustered 7-float boxes with an all-NaN row (n // 5), a NaN x (n // 3), a NaN dx (n // 2) and a NaN yaw (n // 4, which
    NmsNormalGpu never reads).  NmsNormalGpu's fmaxf / fminf drop a NaN edge and, for a NaN size, clamp the NaN union to 1e-8:
    such a box suppresses, and is suppressed by, whatever its remaining extent overlaps.  normal_iou models it."""
    b = normal_from_aligned(clustered_aligned(n, max(2, n // 16), seed)[0], seed)
    b[n // 5] = np.nan
    b[n // 3, 0] = b[n // 2, 3] = b[n // 4, 6] = np.nan
    return b


def rot_nan(n, seed):
    """Clustered rotated boxes with an all-NaN row and rows with a NaN x, dx and yaw: every comparison of the clipping is false,
    the overlap is 0, and such a box neither suppresses nor is suppressed under NmsGpu and boxes_iou_nms_gpu."""
    b = rot_clustered(n, max(4, n // 12), seed)
    b[n // 5] = np.nan
    b[n // 3, 0] = b[n // 2, 3] = b[n // 4, 6] = np.nan
    return b


def circle_clustered(n, nobj, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-50, 50, (nobj, 2))
    return (c[rng.integers(0, nobj, n)] + rng.normal(0, 0.8, (n, 2))).astype(np.float32)


def circle_chain(n, thr, seed):
    rng = np.random.default_rng(seed)
    s = 0.75 * np.sqrt(thr)               # s^2 <= thr < (2 s)^2
    xy = np.stack([np.arange(n - 1) * s - 40.0, rng.uniform(0, 0.01, n - 1)], 1)
    return np.concatenate([[[500.0, 500.0]], xy]).astype(np.float32)


def circle_lattice(seed, n=130):
    """Integer centres; thresh 25: pairs at squared distance exactly 25 ((3,4), (5,0)), 26 and 24 are planted."""
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, 40, (n, 2)) * 3
    for q, (dx, dy) in enumerate([(3, 4), (5, 0), (0, 5), (4, 3), (5, 1), (1, 5), (4, 2), (2, 4)]):
        base = np.array([400 + 40 * q, 700])
        xy[8 * q], xy[8 * q + 65] = base, base + [dx, dy]
    return xy.astype(np.float32)


def normal_from_aligned(b4, seed):
    """Corner boxes -> 7-float boxes (x, y, z, dx, dy, dz, yaw) with that footprint, metres."""
    rng = np.random.default_rng(seed)
    b = np.asarray(b4, np.float64) / 20.0
    out = np.zeros((len(b), 7))
    out[:, 0], out[:, 1] = (b[:, 0] + b[:, 2]) / 2 - 30, (b[:, 1] + b[:, 3]) / 2 - 20
    out[:, 3], out[:, 4] = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    out[:, 2], out[:, 5], out[:, 6] = rng.uniform(-2, 0, len(b)), rng.uniform(1, 2, len(b)), rng.uniform(-3, 3, len(b))
    return out.astype(np.float32)


def normal_lattice(thr):
    """Integer centres and even sizes: footprints with IoU exactly thr (`>`: not suppressed), just above and just below."""
    k = {0.5: 2, 0.25: 4}[thr]
    rows = []
    for r, (a, b) in enumerate([(4, 6), (10, 2), (6, 12)]):
        y = 60 * r
        for x0, wa, wb in [(0, k * a, a), (200, k * a, a + 2), (400, k * a + 2, a)]:
            # both boxes start at x0: centre x0 + w/2
            rows += [[x0 + wa // 2, y, 0, wa, b, 1, 0.3], [x0 + wb // 2, y, 0, wb, b, 1, -0.2]]
    return np.asarray(rows, np.float32)


def rot_clustered(n, nobj, seed, span=40.0):
    """Car-sized boxes (x, y, z, dx, dy, dz, yaw) around nobj objects: position jitter 6 % / size jitter 12 %, yaw jitter, +-pi flips."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-span, span, (nobj, 2))
    yaw = rng.uniform(-np.pi, np.pi, nobj)
    size = np.stack([rng.uniform(3.6, 5.2, nobj), rng.uniform(1.6, 2.1, nobj)], 1)
    o = rng.integers(0, nobj, n)
    b = np.zeros((n, 7))
    b[:, 0:2] = c[o] + rng.normal(0, 0.06, (n, 2)) * size[o]
    b[:, 2] = rng.uniform(-2, 0, n)
    b[:, 3:5] = size[o] * np.exp(rng.normal(0, 0.12, (n, 2)))
    b[:, 5] = rng.uniform(1.4, 1.8, n)
    b[:, 6] = yaw[o] + rng.normal(0, 0.08, n) + np.pi * rng.integers(-1, 2, n)
    return b.astype(np.float32)


def rot_chain(n, thr, seed, length=4.5, width=1.9):
    """Boxes strung along their own long axis: neighbours suppress, second neighbours do not (at thr).  Yaw, width and lateral
    position are jittered a little: exactly parallel, collinear edges are a degenerate input of the reference's clipping (its
    edge-crossing test is strict) and outside the geometric band."""
    rng = np.random.default_rng(seed)
    yaw = float(rng.uniform(0.2, 1.3))
    s = chain_step(length, thr)
    k = np.arange(n - 1)
    lat = rng.uniform(-0.02, 0.02, n - 1)
    b = np.zeros((n, 7))
    b[1:, 0] = np.cos(yaw) * s * k - np.sin(yaw) * lat - 30
    b[1:, 1] = np.sin(yaw) * s * k + np.cos(yaw) * lat - 30
    b[1:, 6] = yaw + rng.uniform(-0.02, 0.02, n - 1) + np.pi * rng.integers(0, 2, n - 1)
    b[0, 0:2], b[0, 6] = (300.0, 300.0), 0.5
    b[:, 3], b[:, 4], b[:, 5] = length, width, 1.6
    b[1:, 4] += rng.uniform(-0.03, 0.03, n - 1)
    return b.astype(np.float32)


def rot_nested_ties(thr):
    """Yaw-0 boxes on integer and quarter coordinates, one nested in the other without a shared edge line: no edges cross, the
    polygon is the inner box's four corners and every fp32 operation is exact.  Rows 6k, 6k+1: IoU exactly thr (1/2 or 1/4);
    6k+2, 6k+3: the inner box a quarter wider (above thr); 6k+4, 6k+5: a quarter narrower (below)."""
    (W, H), (w, h) = {0.5: ((8, 6), (6, 4)), 0.25: ((8, 4), (4, 2))}[thr]
    rows = []
    for k, (x, y) in enumerate([(0, 0), (-40, 24), (64, -16)]):
        for q, dw in enumerate((0.0, 0.25, -0.25)):
            cx = x + 20 * q
            rows += [[cx, y, -1, W, H, 2, 0], [cx, y, -1, w + dw, h, 2, 0]]
    return np.asarray(rows, np.float32)


def with_zero_tail(b, rows):
    """The list's last `rows` rows all zero, as md_gather_rows leaves the rows past a list's count (CenterPoint)."""
    b = np.array(b, np.float32)
    b[len(b) - rows:] = 0
    return b


def rot_dead_only(n, seed):
    """Only dead boxes: dx = 0 or dy = 0 (or both), anywhere."""
    b = rot_clustered(n, 5, seed)
    k = np.arange(n) % 3
    b[k == 0, 3] = 0
    b[k == 1, 4] = 0
    b[k == 2, 3:5] = 0
    return b


ROT_THRS = (0.2, 0.7)
ROT_NS = (65, 320)


def rot_lists():
    """name -> (boxes, thr): every rotated list the GPU tests run (the CPU tests measure the slack and the undecided share on them)."""
    out = {}
    for n in ROT_NS:
        for thr in ROT_THRS:
            out[f"clustered-{n}-{thr}"] = (rot_clustered(n, max(4, n // 12), 1000 + n), thr)
            out[f"chain-{n}-{thr}"] = (rot_chain(n, thr, 1100 + n), thr)
            out[f"tail-{n}-{thr}"] = (with_zero_tail(rot_clustered(n, max(4, n // 12), 1200 + n), 21), thr)
    out["dead-only-65"] = (rot_dead_only(65, 5), 0.2)
    out["nan-65-0.2"] = (rot_nan(65, 6), 0.2)
    for thr in (0.5, 0.25):
        out[f"nested-{thr}"] = (rot_nested_ties(thr), thr)
    return out


def normal_lists():
    """name -> (boxes[n,7], thr, exact) for NmsNormalGpu."""
    out = {}
    for n in (65, 640):
        for thr in (0.25, 0.5):
            out[f"clustered-{n}-{thr}"] = (normal_from_aligned(clustered_aligned(n, max(2, n // 16), 300 + n)[0], n), thr, False)
            out[f"chain-{n}-{thr}"] = (normal_from_aligned(chain_aligned(n, thr, 310 + n), n + 1), thr, False)
        out[f"nan-{n}-0.5"] = (nan_normal(n, 320 + n), 0.5, False)
    for thr in (0.25, 0.5):
        out[f"lattice-{thr}"] = (normal_lattice(thr), thr, True)
    return out


CIRCLE_THR = 4.0


def circle_lists():
    """name -> (xy[n,2], thresh, exact) for md_circle_nms."""
    out = {}
    for n in (65, 640):
        out[f"clustered-{n}"] = (circle_clustered(n, max(2, n // 16), 400 + n), CIRCLE_THR, False)
        out[f"chain-{n}"] = (circle_chain(n, CIRCLE_THR, 410 + n), CIRCLE_THR, False)
    out["lattice"] = (circle_lattice(7), 25.0, True)
    return out


# md_nms_aligned on four all-zero rows at thr 0.5, eps 0: kept indices per mode (0: 0/0 = NaN, 1: area 1 each and ovr 1, 2: 0 / 1e-8)
ZERO_ROWS_KEPT = {0: [0, 1, 2, 3], 1: [0], 2: [0, 1, 2, 3]}

ALIGNED_THRS = (0.45, 0.5, 0.7)
ALIGNED_NS = (1, 63, 64, 65, 129, 640)


def aligned_batch(n, mode, thr, seed):
    """The six lists of one md_nms_aligned launch at length n: (boxes[6,n,4], count[6], group[6,n], kinds[6])."""
    c5, g5 = clustered_aligned(n, max(1, n // 16), seed, 5)
    c80, g80 = clustered_aligned(n, max(1, n // 8), seed + 1, 80)
    c1, g1 = clustered_aligned(n, max(1, n // 40), seed + 2, 1)
    ch = chain_aligned(n, thr, seed + 3) if n > 1 else c1.copy()
    la = lattice_clustered(n, seed + 4, mode) if n >= 63 else c1.copy()
    ni, gn = nan_inf_aligned(n, seed + 5) if n >= 63 else (c1.copy(), g1)
    boxes = np.stack([c5, c80, c1, ch, la, ni])
    group = np.stack([g5, g80, g1, np.zeros(n, np.int32), np.zeros(n, np.int32), gn]).astype(np.int32)
    # every list kind meets every count over the six lengths; n + 7 is past the list: the kernel clamps it to n
    base = [n, max(n - 5, 0), 64, n + 7, 1, 0]
    r = ALIGNED_NS.index(n)
    count = np.array([base[(i + r) % 6] for i in range(6)], np.int32)
    return boxes, count, group, ["clustered5", "clustered80", "clustered1", "chain", "lattice", "naninf"]


def aligned_full_lists(mode, thr, seed, n=640):
    """Chain, lattice, NaN / inf and an 80-class clustered list at their full length in one launch: (boxes[4,n,4], group[4,n], kinds)."""
    c80, g80 = clustered_aligned(n, n // 8, seed, 80)
    ni, gn = nan_inf_aligned(n, seed + 1)
    boxes = np.stack([chain_aligned(n, thr, seed + 2), lattice_clustered(n, seed + 3, mode), ni, c80])
    group = np.stack([np.zeros(n, np.int32), np.zeros(n, np.int32), gn, g80]).astype(np.int32)
    return boxes, group, ["chain", "lattice", "naninf", "clustered80"]


def quota_prefix_batch(n, quota, seed):
    """Lists around the quota prefix P = roundup64(max(512, 4 quota)) of md_nms_aligned: (boxes[6,n,4], count[6], group[6,n], P).
    0: fills the quota at box P-1.  1: needs box P.  2: the prefix collapses to 3 survivors.  3: shorter than P.  4: clustered,
    class-keyed.  5: empty."""
    P = (max(512, 4 * quota) + 63) // 64 * 64
    rng = np.random.default_rng(seed)

    def filled_at(last):
        # quota - 1 fresh cells first, copies of them up to `last`, where the quota-th fresh cell sits; fresh cells after it
        p = np.concatenate([np.arange(quota - 1), rng.integers(0, quota - 1, last - (quota - 1)), [quota - 1]])
        rest = n - len(p)
        return np.concatenate([p, quota + np.arange(max(rest, 0))])[:n] if rest > 0 else p[:n]

    pats = [filled_at(P - 1), filled_at(P), np.concatenate([rng.integers(0, 3, min(P + 90, n)), 3 + np.arange(max(n - P - 90, 0))])[:n]]
    pats = [np.concatenate([p, np.zeros(n - len(p), int)]) if len(p) < n else p for p in pats]
    lists = [slot_aligned(p, seed + i) for i, p in enumerate(pats)]
    lists.append(slot_aligned(rng.integers(0, 150, n), seed + 3))
    cb, cg = clustered_aligned(n, 140, seed + 4, 80)
    lists.append(cb)
    lists.append(cb.copy())
    group = np.zeros((6, n), np.int32)
    group[4] = cg
    count = np.array([n, n, n, P - 37, n, 0], np.int32)
    return np.stack(lists), count, group, P


def rank_cap_lists(kept=4288, copies=128, first=4100):
    """`kept` disjoint lattice boxes (every one kept, rank = index), then exact copies of the kept boxes of rank first..first+copies-1:
    their suppressors are past SCAN_KEEP_CAP (4288 kept + 128 copies = 4416 boxes: ranks up to 4227 need that many kept ones).
    Returns corner boxes [n,4], circle centres [n,2] and 7-float boxes [n,7]."""
    assert first >= SCAN_KEEP_CAP and first + copies <= kept
    k = np.concatenate([np.arange(kept), first + np.arange(copies)])
    ox, oy = (k % 84) * 24, (k // 84) * 24
    b4 = np.stack([ox + 2, oy + 2, ox + 20, oy + 20], 1).astype(np.float32)
    assert _is_lattice(b4)
    xy = np.stack([ox, oy], 1).astype(np.float32)
    b7 = np.zeros((len(k), 7), np.float32)
    b7[:, 0], b7[:, 1], b7[:, 3], b7[:, 4], b7[:, 5] = ox + 8, oy + 8, 16, 16, 1
    return b4, xy, b7


# ------------------------------------------------------------------------------------------------ soft-NMS
def soft_nms_ref(boxes, scores, n, sigma=0.5, Nt=0.5, threshold=0.001, method=2):
    """md_soft_nms's documented algorithm in float64 on the first n boxes of one list: pick the live maximum (ties go to the
    lowest index), decay every other live box that overlaps it (+1 pixel areas), drop a decayed box whose score fell below
    `threshold` (a box is only ever dropped right after a decay), repeat until nothing is live.

    Returns dict(order, scores, ndecay, tol, violations).  scores[i] = final score of box i if it was selected, else 0.  tol[i]
    bounds |fp32 - float64| of that score; per decay of a score s by a weight w:  tol' = s dw + w tol + u w s  with
        overlap ov: the 25 u relative of the aligned band's derivation (5 on the intersection, 19 on the union, 1 on the quotient)
        method 1: dw = 25 u ov + u above Nt, else 0        method 3: dw = 0
        method 2: w = expf(-(ov ov) / sigma): the argument x carries 2 * 25 + 2 u relative, expf itself at most one ulp:
                  dw = w (52 u x + 2 u)
    violations counts the places where fp32 could decide differently from float64, so that the order is an equality when it is
    0: two live scores at a pick closer than their tolerances (exact ties between never-decayed boxes are decided by index and
    are allowed), an overlap within its band of Nt (methods 1, 3), a score within its tolerance of `threshold` at a drop, and an
    intersection extent within 2^-9 of 0 (|coordinates| < 2^12: two roundings of at most 2^-11 each; with every coordinate on
    the 1/8 grid the extents are exact and none is counted)."""
    b = np.asarray(boxes, np.float32).astype(np.float64)[:n]
    s = np.asarray(scores, np.float32).astype(np.float64)[:n].copy()
    assert n == 0 or np.abs(b).max() < 2 ** 12
    clear = 0.0 if (b * 8 == np.round(b * 8)).all() else 2.0 ** -9
    Nt, threshold, sigma = thr64(Nt), thr64(threshold), thr64(sigma)
    tol = np.zeros(n)
    ndecay = np.zeros(n, np.int64)
    state = np.zeros(n, np.int8)   # 0 live, 1 selected, 2 removed
    area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    order, violations = [], 0
    while True:
        live = np.nonzero(state == 0)[0]
        if live.size == 0:
            break
        best = live[np.argmax(s[live])]            # argmax returns the first maximum: the lowest index
        other = live[live != best]
        close = np.abs(s[other] - s[best]) <= tol[other] + tol[best]
        exact_tie = (tol[other] == 0) & (tol[best] == 0)
        violations += int((close & ~exact_tie).sum())
        state[best] = 1
        order.append(int(best))
        if other.size == 0:
            continue
        t = b[best]
        iw = np.minimum(t[2], b[other, 2]) - np.maximum(t[0], b[other, 0]) + 1
        ih = np.minimum(t[3], b[other, 3]) - np.maximum(t[1], b[other, 1]) + 1
        violations += int((np.abs(iw) < clear).sum() + ((iw > 0) & (np.abs(ih) < clear)).sum())
        hit = (iw > 0) & (ih > 0)
        o = other[hit]
        inter = iw[hit] * ih[hit]
        ov = inter / (area[best] + area[o] - inter)
        if method == 2:
            x = ov * ov / sigma
            w = np.exp(-x)
            dw = w * (52 * U * x + 2 * U)
        else:
            above = ov > Nt
            violations += int((np.abs(ov - Nt) <= 25 * U * ov + U * Nt).sum())
            w = np.where(above, 1 - ov if method == 1 else 0.0, 1.0)
            dw = np.where(above & (method == 1), 25 * U * ov + U, 0.0)
        tol[o] = s[o] * dw + w * tol[o] + U * w * s[o] * (dw > 0)
        s[o] = w * s[o]
        ndecay[o] += 1
        violations += int((np.abs(s[o] - threshold) <= tol[o] + U * threshold).sum())
        state[o[s[o] < threshold]] = 2
    out = np.where(state == 1, s, 0.0)
    return dict(order=np.asarray(order, np.int64), scores=out, ndecay=ndecay, tol=tol, violations=violations)


def soft_nms_list(n, seed, ties=0, field=None):
    """n boxes (10..80 pixels in a field that grows with n), distinct scores; the last `ties` boxes are isolated (disjoint from
    everything, never decayed) and share one score in pairs: planted exact ties."""
    rng = np.random.default_rng(seed)
    m = n - ties
    # the field grows with n (and is sparser past 300 boxes, where a box would otherwise take hundreds of decays and the score
    # tolerances would close every gap between live scores)
    W = field or 200.0 * max(1.0, np.sqrt(m / 100.0)) * (2.5 if m > 300 else 1.0)
    cx, cy = rng.uniform(0, W, m), rng.uniform(0, 0.75 * W, m)
    w, h = rng.uniform(10, 80, m), rng.uniform(10, 80, m)
    boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    scores = rng.uniform(0.01, 1, m) + np.arange(m) * 1e-6
    if ties:
        k = np.arange(ties)
        iso = np.stack([100.0 * k, np.full(ties, 3000.0), 100.0 * k + 50, np.full(ties, 3040.0)], 1)
        boxes = np.concatenate([boxes, iso])
        scores = np.concatenate([scores, 0.3 + 0.2 * (k // 2)])
        perm = rng.permutation(n)
        boxes, scores = boxes[perm], scores[perm]
    # coordinates on a 1/8 pixel grid below 2^12: every intersection extent is exact in fp32, its sign is not in question
    return (np.round(boxes * 8) / 8).astype(np.float32), scores.astype(np.float32)


def soft_nms_case(n, method, seed, ties=0, threshold=0.001, count=None):
    """(boxes, scores, reference) drawn, and re-drawn from the next seed, until the reference (on the first `count` boxes) has no
    violation."""
    for k in range(64):
        boxes, scores = soft_nms_list(n, seed + k, ties)
        ref = soft_nms_ref(boxes, scores, n if count is None else min(count, n), method=method, threshold=threshold)
        if ref["violations"] == 0:
            return boxes, scores, ref
    raise AssertionError("no clear soft-NMS list in 64 draws")


SOFT_NS = (1, 64, 65, 300, 1024)
SOFT_METHODS = (1, 2, 3)


def soft_cases():
    """(n, method, seed, ties, threshold) of every md_soft_nms list the GPU tests run: the reference call's threshold 0.001, and
    lists with planted exact score ties at threshold 0.05, where methods 1 and 2 drop boxes too."""
    out = [(n, m, 7000 + 10 * n + m, 0, 0.001) for n in SOFT_NS for m in SOFT_METHODS]
    out += [(n, m, 9000 + 10 * n + m, 6, 0.05) for n in (65, 300) for m in SOFT_METHODS]
    return out


def soft_tolerance(ref):
    """Per-box score tolerance of a device run against soft_nms_ref: the derived bound, and never looser than the 2e-6 max(1, |s|)
    of tests/test_detops_gpu.py::test_soft_nms_vs_published_algorithm."""
    return np.minimum(ref["tol"], 2e-6 * np.maximum(1.0, np.abs(ref["scores"]))) + 2.0 ** -149
