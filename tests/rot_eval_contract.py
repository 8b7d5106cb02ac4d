"""Float64 geometric contract of the KITTI rotated overlap (csrc/rot_eval.h's rie_pair behind md_rotate_iou_eval and metrics 1 and 2
of md_kitti_eval_overlaps): the judge, seeded pair generators, measured bands, the AP set.  numpy, CPU only; imports neither the
product nor the oracle.

rie_pair, oracle/det_oracle.c's orc_rotate_iou_eval_pair and kitti_eval.py's column picks restate one reading of the reference's
numba-CUDA kernel; a misreading shared by the three (corner order, the sign of ry, l against w, which operand a criterion divides
by, the [y - h, y] interval) passes every comparison among them.  The judge below is built from the KITTI definition of a box
instead and from the convex clipper of tests/nms_contract.py, and never from that kernel's code.

The judge (float64 on the fp32-rounded BEV columns):
    a BEV box (x, z, l, w, ry) has heading (cos ry, -sin ry) in the x-z plane, half-extent l/2 along it and w/2 across it;
    ai = area of the intersection of the two rectangles (nms_contract.clip_area);  a1 = l w of the `boxes` operand, a2 of `query`
    criterion -1: ai / (a1 + a2 - ai)    0: ai / a1    1: ai / a2    anything else: ai
    a camera box (x, y, z, l, h, w, ry) has its bottom face at y and -y pointing up: it spans [y - h, y].  judge_3d = ai ih / (v1 + v2 -
    ai ih) with ih the overlap of the two intervals and v = l h w, 0 where ai or ih is not positive.  Heights and volumes are taken
    in float64 as given (the product keeps them in float64 too); only the five BEV columns are rounded to fp32.

Operand order.  rie_pair(r1 = boxes row, r2 = query row) divides by the area of `boxes` under criterion 0 and that is what the judge
states.  The reference's driver (rotate_iou.py:298-302) hands devRotateIoUEval the QUERY box first, so its criterion 0 divides by the
query's area and its criterion 1 by the boxes': for 0 and 1 the product has the operands the other way round than the numba kernel.
The evaluator only ever asks for -1 (BEV) and 2 (3D), which are symmetric, so no AP depends on it; it is recorded here, not changed.

Excursion of an fp32 value v from the judge j:  |v - j| for criterion -1, 0, 1;  |v - j| / (1 + j) for criterion 2.
Bands.  Per generator g two numbers, measured on the fp32 CPU oracle (oracle.rotate_iou_eval) over the four criteria and recorded
below (tests/test_rot_eval_contract_cpu.py re-measures them: measured <= recorded <= 2 x measured): W_g the worst excursion, Q_g the
99.9th percentile ("higher" rule) of the excursion over the LIVE pairs, those with j > 0 or v != 0 -- the many disjoint pairs of an
N x K call, exact zeros on both sides, would otherwise let the percentile say nothing.  A device result fits when every pair is
within 4 W_g and at most 1 live pair in 1000 is beyond 4 Q_g.  The factor 4 (that of nms_contract.ROT_SLACK): the device's cosf / sinf
differ from glibc's in the last bits, which moves a corner by about an ulp of its coordinate, the order of the roundings W_g already
holds.  The bands are never taken from a device result.
3D band.  With V = v1 + v2, v(a) = a ih / (V - a ih) and  v(a + e) - v(a) = ih e V / ((V - a ih)(V - (a + e) ih)):  an area
excursion of at most e = w (1 + ai) gives |dv| <= ih e V / (U (U - ih e)), U = V - ai ih (band_3d); where ih <= 0 the value is exactly 0.

The coincident regime is outside the geometric argument and outside every band above.  The reference's corner test
(rotate_iou.py:164-179, point_in_quadrilateral) is non-strict fp32 `>=` and its crossing test strict `>`: when corners of one box lie
on the edges of the other the roundings decide which vertices the polygon gets, and it loses area.  Share of pairs whose oracle IoU
is below 0.99 of the true one (257 car-sized pairs per sub-case, COINCIDENT_SHARE below; tests/test_rot_eval_contract_cpu.py
re-measures and prints them):
    bit-identical boxes, arbitrary yaw                          0.9883 (the IoU comes out as 0 or about 1/3)
    bit-identical, yaw in {+-float32(1.57), float32(pi)}        0.7471
    bit-identical, yaw exactly 0                                0: the trig is exact and every comparison an equality
    equal yaw, one shared edge line                             0.1362
With bit-identical boxes the polygon is built from a subset of the true vertices and only loses area.  With a shared edge line the
reference's arithmetic does not: the strict crossing test of the two collinear edges is decided by rounding, and where it says
"crossing" the point is a quotient of two rounding residues, anywhere in the plane.  Restated literally, 93 of the 257 shared-edge
pairs exceeded the true value on the oracle (97 on an MI355X): intersection areas up to 672 m2 for 6 m2 cars, criterion -1 from -34.6
to +30.8, and 0.3230 of the pairs below 0.99 of the truth.  That was wrong by any reading, and rie_pair and the oracle now keep a
crossing only if it lies on both segments within 2^-16 of the largest coordinate (csrc/rot_eval.h, RIE_CROSS_TOL).  With it the range
condition of the device test (finite, within [0, judge + 4 W]) holds in all four sub-cases; every pair of the generators above keeps its
bits, and so do the three bit-identical sub-cases.
The loss of area is the reference's behaviour and stays: evaluating a result set against a bit-identical copy of itself is not a sanity check this
metric supports unless every yaw is 0.
"""
import functools

import numpy as np

from tests import nms_contract as nc

N = 257                                   # boxes and queries per generator: one more than the 256-lane workgroup
CRITERIA = (-1, 0, 1, 2)
CLASS_SIZE = {"car": (3.9, 1.6), "pedestrian": (0.8, 0.6), "cyclist": (1.76, 0.6)}       # l, w
CLASS_HEIGHT = {"car": 1.5, "pedestrian": 1.7, "cyclist": 1.7}
CENTRE_SIGMA = {"car": 0.3, "pedestrian": 0.1, "cyclist": 0.3}

# W_g, Q_g: worst and 99.9th-percentile excursion of oracle.rotate_iou_eval from the judge over the generator's 257 x 257 pairs and
# the four criteria; the measured value stands beside each (test_bands_are_the_measured_ones re-measures)
BANDS = {
    "kitti_jitter_car": (1.13e-4, 6.02e-5),         # measured 1.127e-4, 6.019e-5
    "kitti_jitter_pedestrian": (1.14e-3, 6.25e-4),  # measured 1.130e-3, 6.244e-4
    "kitti_jitter_cyclist": (1.50e-4, 1.40e-4),     # measured 1.491e-4, 1.396e-4
    "near_parallel": (1.06e-4, 5.78e-5),            # measured 1.053e-4, 5.773e-5
    "same_yaw_shifted": (4.04e-5, 4.04e-5),         # measured 4.034e-5 twice: 293 live pairs, the percentile is the worst
    "nested": (1.68e-5, 1.68e-5),                   # measured 1.675e-5 twice (257 live pairs)
    "crossed": (2.24e-5, 2.24e-5),                  # measured 2.231e-5 twice (257 live pairs)
    "far": (0.0, 0.0),                              # measured 0, 0: every pair disjoint, exact zeros
    "uniform_10": (2.04e-6, 1.62e-6),               # measured 2.032e-6, 1.619e-6 (700 x 45 pairs, 2653 of them live)
}
BAND_FACTOR = 4
# share of bit-coincident pairs whose oracle IoU is below 0.99 of the true IoU (test_coincident_shares_are_the_recorded_ones)
COINCIDENT_SHARE = {"identical": 0.9883, "identical_quarter": 0.7471, "identical_yaw0": 0.0, "shared_edge": 0.1362}


# ------------------------------------------------------------------------------------------------ the judge
def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def bev_corners(b5):
    """[m,5] (x, z, l, w, ry) float64 -> [m,4,2] corners, counter-clockwise in the (x, z) plane."""
    b = np.asarray(b5, np.float64).reshape(-1, 5)
    c, s = np.cos(b[:, 4]), np.sin(b[:, 4])
    head = np.stack([c, -s], 1)                        # the heading; `side` is the heading turned by +90 degrees
    side = np.stack([s, c], 1)
    sl, sw = np.array([-1.0, 1.0, 1.0, -1.0]), np.array([-1.0, -1.0, 1.0, 1.0])
    along = (sl[None, :] * b[:, 2:3] / 2)[..., None] * head[:, None, :]
    across = (sw[None, :] * b[:, 3:4] / 2)[..., None] * side[:, None, :]
    return b[:, None, 0:2] + along + across


def judge_area(boxes5, query5):
    """[N,K] float64 area of the intersection of every boxes rectangle with every query rectangle."""
    b, q = _f32(boxes5).reshape(-1, 5), _f32(query5).reshape(-1, 5)
    out = np.zeros((len(b), len(q)))
    if out.size == 0:
        return out
    # rectangles whose centres are further apart than the sum of their half-diagonals are disjoint: exactly 0, nothing to clip
    rb, rq = np.hypot(b[:, 2], b[:, 3]) / 2, np.hypot(q[:, 2], q[:, 3]) / 2
    d = np.hypot(b[:, None, 0] - q[None, :, 0], b[:, None, 1] - q[None, :, 1])
    i, j = np.nonzero(d <= (rb[:, None] + rq[None, :]) * (1 + 1e-9))
    if i.size:
        out[i, j] = nc.clip_area(bev_corners(b[i]), bev_corners(q[j]))
    return out


def criterion_value(ai, a1, a2, criterion):
    with np.errstate(all="ignore"):
        if criterion == -1:
            return ai / (a1 + a2 - ai)
        if criterion == 0:
            return ai / (a1 + 0 * a2)
        if criterion == 1:
            return ai / (a2 + 0 * a1)
    return ai


def judge_bev(boxes5, query5, criterion=-1, area=None):
    """[N,K]: criterion -1 IoU, 0 ai / area of the boxes operand, 1 ai / area of the query operand, else ai.  `area`: a judge_area
    of the same operands computed earlier."""
    b, q = _f32(boxes5).reshape(-1, 5), _f32(query5).reshape(-1, 5)
    ai = judge_area(b, q) if area is None else area
    return criterion_value(ai, (b[:, 2] * b[:, 3])[:, None], (q[:, 2] * q[:, 3])[None, :], criterion)


def judge_3d(cam_boxes7, cam_query7, parts=False):
    """[N,K] 3D IoU of camera boxes (x, y, z, l, h, w, ry); parts=True: also (ai, ih, v1 + v2) for band_3d."""
    b, q = np.asarray(cam_boxes7, np.float64).reshape(-1, 7), np.asarray(cam_query7, np.float64).reshape(-1, 7)
    ai = judge_area(b[:, [0, 2, 3, 5, 6]], q[:, [0, 2, 3, 5, 6]])
    top = np.maximum((b[:, 1] - b[:, 4])[:, None], (q[:, 1] - q[:, 4])[None, :])
    ih = np.minimum(b[:, None, 1], q[None, :, 1]) - top
    vsum = (b[:, 3] * b[:, 4] * b[:, 5])[:, None] + (q[:, 3] * q[:, 4] * q[:, 5])[None, :]
    inc = ai * ih
    with np.errstate(all="ignore"):
        v = np.where((ai > 0) & (ih > 0), inc / (vsum - inc), 0.0)
    return (v, ai, ih, vsum) if parts else v


def band_3d(ai, ih, vsum, w):
    """Bound of |3D value - judge_3d| when the BEV area is within w (1 + ai) of ai (the derivation is in the module docstring)."""
    e = w * (1 + ai)
    u = vsum - ai * ih
    den = u * (u - ih * e)
    with np.errstate(all="ignore"):
        return np.where(ih > 0, np.where(den > 0, ih * e * vsum / den, np.inf), 0.0)


def excursion(value, judge, criterion):
    d = np.abs(np.asarray(value, np.float64) - judge)
    return d / (1 + judge) if criterion == 2 else d


def live(value, judge):
    return (judge > 0) | (np.asarray(value) != 0)


def percentile_999(x):
    return float(np.percentile(x, 99.9, method="higher")) if x.size else 0.0


def band_report(value, judge, criterion, name):
    """(worst excursion / (4 W), live pairs beyond 4 Q, live pairs) of an fp32 result against the judge under BANDS[name]."""
    w, q = BANDS[name]
    exc = excursion(value, judge, criterion)
    lv = live(value, judge)
    worst = float(exc.max()) if exc.size else 0.0
    frac = worst / (BAND_FACTOR * w) if w > 0 else (0.0 if worst == 0 else np.inf)
    return frac, int((exc[lv] > BAND_FACTOR * q).sum()), int(lv.sum())


def fits(value, judge, criterion, name):
    value = np.asarray(value)
    frac, beyond, n = band_report(value, judge, criterion, name)
    return bool(np.isfinite(value).all()) and frac <= 1.0 and beyond * 1000 <= n


# ------------------------------------------------------------------------------------------------ generators (all seeded)
def _cluster_centres(rng, n, spread, nclusters=30):
    c = np.stack([rng.uniform(-38, 38, nclusters), rng.uniform(3, 77, nclusters)], 1)
    return c[rng.integers(0, nclusters, n)] + rng.normal(0, spread, (n, 2))


def _grid_centres(rng, n, lo=-40.0):
    """n of the 17 x 16 cells (4.7 m x 5.0 m) of x in [lo, lo + 79.9], z in [0, 80], in a random order: boxes with a
    half-diagonal under 2.3 m in different cells are disjoint"""
    cell = rng.permutation(17 * 16)[:n]
    x = lo + 4.7 * (cell % 17 + 0.5) + rng.uniform(-0.02, 0.02, n)
    z = 5.0 * (cell // 17 + 0.5) + rng.uniform(-0.02, 0.02, n)
    return np.stack([x, z], 1)


def _truths(rng, centres, l, w):
    n = len(centres)
    size = np.array([l, w]) * rng.uniform(0.9, 1.1, (n, 2))
    return np.concatenate([centres, size, rng.uniform(-np.pi, np.pi, (n, 1))], 1)


def _pair(b, q):
    return np.ascontiguousarray(b, np.float32), np.ascontiguousarray(q, np.float32)


def kitti_jitter(cls, seed=None, n=N):
    """Ground truths of one class in about 30 clusters inside x +-40, z 0-80 (so that off-diagonal pairs overlap too); query i is
    ground truth i with centre + N(0, 0.3 m; 0.1 m for pedestrians), size x U(0.9, 1.1), yaw + N(0, 0.05)."""
    l, w = CLASS_SIZE[cls]
    rng = np.random.default_rng(4100 + list(CLASS_SIZE).index(cls) if seed is None else seed)
    b = _truths(rng, _cluster_centres(rng, n, 0.4 * l), l, w)
    q = b.copy()
    q[:, 0:2] += rng.normal(0, CENTRE_SIGMA[cls], (n, 2))
    q[:, 2:4] *= rng.uniform(0.9, 1.1, (n, 2))
    q[:, 4] += rng.normal(0, 0.05, n)
    return _pair(b, q)


def near_parallel(n=N):
    """As the cars, but the yaw differs by N(0, 1e-3), and never by less than 1e-5: near-parallel edges, never parallel ones."""
    rng = np.random.default_rng(4200)
    l, w = CLASS_SIZE["car"]
    b = _truths(rng, _cluster_centres(rng, n, 0.4 * l), l, w)
    q = b.copy()
    q[:, 0:2] += rng.normal(0, 0.3, (n, 2))
    q[:, 2:4] *= rng.uniform(0.9, 1.1, (n, 2))
    d = rng.normal(0, 1e-3, n)
    q[:, 4] += np.where(np.abs(d) < 1e-5, np.copysign(1e-5, d), d)
    return _pair(b, q)


def same_yaw_shifted(n=N):
    """Exactly equal yaw, different sizes, the centre shifted by 0.3-1.2 m along and 0.15-0.6 m across the box: the size differences
    are at most 0.2 m and 0.09 m per side, so no two edge lines coincide.  On the grid: only pair (i, i) overlaps."""
    rng = np.random.default_rng(4300)
    l, w = CLASS_SIZE["car"]
    b = _truths(rng, _grid_centres(rng, n), l, w).astype(np.float32).astype(np.float64)
    q = b.copy()
    q[:, 2:4] *= rng.uniform(0.9, 1.1, (n, 2))
    du = rng.uniform(0.3, 1.2, n) * rng.choice([-1.0, 1.0], n)
    dv = rng.uniform(0.15, 0.6, n) * rng.choice([-1.0, 1.0], n)
    c, s = np.cos(b[:, 4]), np.sin(b[:, 4])
    q[:, 0] += du * c + dv * s
    q[:, 1] += -du * s + dv * c
    return _pair(b, q)


def nested(n=N):
    """A small box (0.5-1.0 m x 0.3-0.6 m) at any yaw inside a car, at least 0.1 m from every side: the circle around its centre
    through its corners stays 0.1 m inside.  Even i: the car is the boxes operand, odd i: the query.  The intersection is the small
    box: four corners, no crossing.  On the grid."""
    rng = np.random.default_rng(4400)
    l, w = CLASS_SIZE["car"]
    outer = _truths(rng, _grid_centres(rng, n), l, w)
    inner = np.zeros((n, 5))
    inner[:, 2], inner[:, 3] = rng.uniform(0.5, 1.0, n), rng.uniform(0.3, 0.6, n)
    r = np.hypot(inner[:, 2], inner[:, 3]) / 2
    du = rng.uniform(-1, 1, n) * (outer[:, 2] / 2 - 0.1 - r)
    dv = rng.uniform(-1, 1, n) * (outer[:, 3] / 2 - 0.1 - r)
    assert (outer[:, 3] / 2 - 0.1 - r > 0.02).all()
    c, s = np.cos(outer[:, 4]), np.sin(outer[:, 4])
    inner[:, 0] = outer[:, 0] + du * c + dv * s
    inner[:, 1] = outer[:, 1] - du * s + dv * c
    inner[:, 4] = outer[:, 4] + rng.uniform(-np.pi, np.pi, n)
    odd = (np.arange(n) % 2 == 1)[:, None]
    return _pair(np.where(odd, inner, outer), np.where(odd, outer, inner))


def crossed(n=N):
    """Long thin boxes (3.6-4.4 m x 0.27-0.33 m) through a common centre region (offset up to 0.5 m), yaw differing by 60-120
    degrees: four crossings, no corner of one inside the other.  On the grid."""
    rng = np.random.default_rng(4500)
    b = _truths(rng, _grid_centres(rng, n), 4.0, 0.3)
    q = b.copy()
    q[:, 0:2] += rng.uniform(-0.5, 0.5, (n, 2))
    q[:, 2:4] *= rng.uniform(0.9, 1.1, (n, 2))
    q[:, 4] += np.deg2rad(rng.uniform(60, 120, n)) * rng.choice([-1.0, 1.0], n)
    return _pair(b, q)


def far(n=N):
    """Every pair disjoint by more than 1 m: boxes left of x = -0.55 by their half-diagonal and more, queries right of x = +0.55."""
    rng = np.random.default_rng(4600)
    l, w = CLASS_SIZE["car"]
    b = _truths(rng, np.zeros((n, 2)), l, w)
    q = _truths(rng, np.zeros((n, 2)), l, w)
    for a, sign in ((b, -1.0), (q, 1.0)):
        a[:, 0] = sign * (0.56 + np.hypot(a[:, 2], a[:, 3]) / 2 + np.abs(rng.normal(0, 6.0, n)))
        a[:, 1] = rng.uniform(0, 80, n)
    return _pair(b, q)


def coincident(n=N):
    """name -> (boxes, query): the regime outside the geometric argument, kept apart from GENERATORS.  On the grid, so pair (i, i) is
    the coincident one and every other pair is disjoint."""
    rng = np.random.default_rng(4700)
    l, w = CLASS_SIZE["car"]
    out = {}
    b = _truths(rng, _grid_centres(rng, n), l, w).astype(np.float32)
    out["identical"] = (b, b.copy())
    b = _truths(rng, _grid_centres(rng, n), l, w).astype(np.float32)
    b[:, 4] = np.array([1.57, -1.57, np.pi], np.float32)[rng.integers(0, 3, n)]
    out["identical_quarter"] = (b, b.copy())
    b = _truths(rng, _grid_centres(rng, n), l, w).astype(np.float32)
    b[:, 4] = 0
    out["identical_yaw0"] = (b, b.copy())
    b = _truths(rng, _grid_centres(rng, n), l, w).astype(np.float32).astype(np.float64)
    q = b.copy()
    q[:, 2] = b[:, 2] * rng.uniform(0.6, 0.9, n)
    q[:, 3] = b[:, 3] * rng.uniform(0.6, 0.9, n)
    du = (b[:, 2] - q[:, 2]) / 2                     # the query's front edge on the line of the box's front edge
    dv = rng.uniform(-0.5, 0.5, n) * (b[:, 3] - q[:, 3]) / 2
    c, s = np.cos(b[:, 4]), np.sin(b[:, 4])
    q[:, 0] += du * c + dv * s
    q[:, 1] += -du * s + dv * c
    out["shared_edge"] = _pair(b, q)
    return out


def uniform_10(n=700, k=45):
    """The set of tests/test_nms_iou_gpu.py::test_rotate_iou_eval_vs_oracle, by its draws: 700 x 45 boxes of 1-5 m, uniform within
    +-10 m and in yaw.  Most pairs are disjoint and none is a detection on its box: it covers the launch, not the evaluator's regime."""
    rng = np.random.default_rng(31)
    b = np.concatenate([rng.uniform(-10, 10, (n, 2)), rng.uniform(1, 5, (n, 2)), rng.uniform(-np.pi, np.pi, (n, 1))], 1).astype(np.float32)
    q = np.concatenate([rng.uniform(-10, 10, (k, 2)), rng.uniform(1, 5, (k, 2)), rng.uniform(-np.pi, np.pi, (k, 1))], 1).astype(np.float32)
    return b, q


GENERATORS = {
    "kitti_jitter_car": lambda: kitti_jitter("car"),
    "kitti_jitter_pedestrian": lambda: kitti_jitter("pedestrian"),
    "kitti_jitter_cyclist": lambda: kitti_jitter("cyclist"),
    "near_parallel": near_parallel,
    "same_yaw_shifted": same_yaw_shifted,
    "nested": nested,
    "crossed": crossed,
    "far": far,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(boxes, query, judge_area, {criterion: judge}) of a generator, of uniform_10 or of coincident()'s `coincident/<sub-case>`;
    computed once."""
    if name.startswith("coincident/"):
        b, q = coincident()[name.split("/", 1)[1]]
    else:
        b, q = uniform_10() if name == "uniform_10" else GENERATORS[name]()
    area = judge_area(b, q)
    for a in (b, q, area):
        a.setflags(write=False)
    return b, q, area, {c: judge_bev(b, q, c, area) for c in CRITERIA}


# ------------------------------------------------------------------------------------------------ the AP set
AP_NAMES = ("Car", "Pedestrian", "Cyclist")
AP_THRESHOLDS = (0.7, 0.5, 0.25)           # every min_overlap of the evaluator's table for the three classes
AP_SEED = 7


def ap_band_w(names_a, names_b):
    """[A,B] the W of the pair's band: the larger of the two classes' kitti_jitter bands"""
    w = {n: BANDS["kitti_jitter_" + n.lower()][0] for n in AP_NAMES}
    return np.maximum(np.array([w[str(n)] for n in names_a])[:, None], np.array([w[str(n)] for n in names_b])[None, :])


def cam_boxes(a):
    return np.concatenate([np.asarray(a["location"], np.float64).reshape(-1, 3), np.asarray(a["dimensions"], np.float64).reshape(-1, 3),
                           np.asarray(a["rotation_y"], np.float64).reshape(-1, 1)], 1)


def ap_margins(gt, dt):
    """Per image and metric the distance of every (detection, ground truth) overlap of the judge from the nearest evaluator
    threshold minus the pair's band (4 W; the 3D one through band_3d): positive = no fp32 result inside the band can change the
    side.  -> (list of [D,G] margins for BEV, the same for 3D, number of overlapping pairs)"""
    bev, d3, overlapping = [], [], 0
    thr = np.array(AP_THRESHOLDS)
    for g, d in zip(gt, dt):
        cg, cd = cam_boxes(g), cam_boxes(d)
        w = BAND_FACTOR * ap_band_w(d["name"], g["name"])
        v1 = judge_bev(cd[:, [0, 2, 3, 5, 6]], cg[:, [0, 2, 3, 5, 6]], -1)
        v3, ai, ih, vsum = judge_3d(cd, cg, parts=True)
        bev.append(np.abs(v1[..., None] - thr).min(-1) - w)
        d3.append(np.abs(v3[..., None] - thr).min(-1) - band_3d(ai, ih, vsum, w))
        overlapping += int((v1 > 0).sum())
    return bev, d3, overlapping


def _objects(rng, names):
    """tests/test_kitti_eval_gpu.py::_annos' construction for the given class names (sizes of the class x U(0.9, 1.1))"""
    n = len(names)
    loc = np.stack([rng.uniform(-15, 15, n), np.full(n, 1.6), rng.uniform(5, 45, n)], 1)
    base = np.array([[CLASS_SIZE[c.lower()][0], CLASS_HEIGHT[c.lower()], CLASS_SIZE[c.lower()][1]] for c in names]).reshape(n, 3)
    dims = base * rng.uniform(0.9, 1.1, (n, 3))
    u = 600 + 700 * loc[:, 0] / loc[:, 2]
    half = 700 * 2.0 / loc[:, 2]
    bbox = np.stack([u - half, 180 - 40 - 600 / loc[:, 2], u + half, 180 + 600 / loc[:, 2]], 1)
    return dict(name=np.array(list(names), dtype=str), bbox=bbox, location=loc, dimensions=dims,
                rotation_y=rng.uniform(-3, 3, n), occluded=rng.integers(0, 3, n), truncated=rng.choice([0.0, 0.2, 0.4], n),
                alpha=rng.uniform(-3, 3, n))


def _jittered_detection(rng, g, i, sigma):
    """object i of annotation g as a one-row detection: centre + N(0, sigma) in x and z, bottom face + N(0, 0.05), size x U(0.9, 1.1)
    (the height included), yaw + N(0, 0.05)"""
    d = {k: np.array(v[i:i + 1]) for k, v in g.items()}
    d["location"] = d["location"] + rng.normal(0, [sigma, 0.05, sigma], (1, 3))
    d["dimensions"] = d["dimensions"] * rng.uniform(0.9, 1.1, (1, 3))
    d["rotation_y"] = d["rotation_y"] + rng.normal(0, 0.05, 1)
    d["bbox"] = d["bbox"] + rng.normal(0, 2.0, (1, 4))
    d["score"] = rng.uniform(0.1, 1.0, 1)
    return d


def _stack(rows, like):
    return {k: np.concatenate([r[k] for r in rows], 0) for k in list(like) + ["score"]}


@functools.lru_cache(maxsize=None)
def ap_set(seed=AP_SEED, images=40):
    """(gt_annos, dt_annos): `images` images of 1-6 objects of the three classes; the detections are the ground truths jittered (centre
    sigma 0.4 m) plus one stray per image, a ground truth of the image displaced with sigma 0.8 m.  A detection whose judged BEV or 3D
    overlap with a ground truth of its image lies within the band of an evaluator threshold is drawn again (from the same seeded
    stream), so that the AP tables of any in-band overlap source are those of the judge: ap_margins(...) is positive everywhere."""
    rng = np.random.default_rng(seed)
    gt, dt = [], []
    for _ in range(images):
        g = _objects(rng, [AP_NAMES[k] for k in rng.integers(0, 3, int(rng.integers(1, 7)))])
        rows = []
        n = len(g["name"])
        for i, sigma in [(i, 0.4) for i in range(n)] + [(int(rng.integers(0, n)), 0.8)]:
            for _try in range(200):
                d = _jittered_detection(rng, g, i, sigma)
                b, t, _ = ap_margins([g], [d])
                if (b[0] > 0).all() and (t[0] > 0).all():
                    break
            else:
                raise AssertionError("no detection clear of the thresholds in 200 draws")
            rows.append(d)
        gt.append(g)
        dt.append(_stack(rows, g))
    return gt, dt


def ap_min_overlaps():
    """[2, 3, 3]: the evaluator's table (0.7 / 0.5 / 0.5 and 0.5 / 0.25 / 0.25 for BEV and 3D) for Car, Pedestrian, Cyclist"""
    return np.array([[[0.7, 0.5, 0.5]] * 3, [[0.7, 0.5, 0.5], [0.5, 0.25, 0.25], [0.5, 0.25, 0.25]]])


def objects(rng, names):
    """Public face of the AP set's object maker, for the extra overlap blocks of the device test."""
    return _objects(rng, names)


def detections_on(rng, g, k, extra_names):
    """Detections for ground truth annotation g: its first k objects jittered (sigma 0.1 m), then fresh objects of extra_names."""
    rows = [_jittered_detection(rng, g, i, 0.1) for i in range(k)]
    e = _objects(rng, extra_names)
    e["score"] = rng.uniform(0.1, 1.0, len(extra_names))
    rows.append(e)
    return _stack(rows, g)
