"""The contract of tests/rot_eval_contract.py, pinned without a GPU: the float64 judge on closed forms, the bands re-measured on the
fp32 CPU oracle (oracle.rotate_iou_eval), the generators' stated conditions, the AP set's distance from every evaluator threshold,
and the evaluator's tables with the judge's overlaps against those with the oracle's.  tests/test_rot_eval_gpu.py holds the device
to the same judge and bands."""
import functools

import numpy as np
import pytest

import oracle
from minddet_amd import kitti_eval as ke
from tests import rot_eval_contract as rc


def _oracle(b, q, criterion):
    return oracle.rotate_iou_eval(np.ascontiguousarray(b, np.float32), np.ascontiguousarray(q, np.float32), criterion)


def _one(b, q, criterion=2):
    return float(rc.judge_bev(np.array([b], np.float64), np.array([q], np.float64), criterion)[0, 0])


# ------------------------------------------------------------------------------------------------ the judge
def test_judge_closed_forms():
    rt2 = np.sqrt(2.0)
    # axis-aligned: l runs along x at ry = 0, w along z
    assert _one([0, 0, 4, 2, 0], [1, 0.5, 4, 2, 0]) == pytest.approx(3 * 1.5, abs=1e-12)
    assert _one([0, 0, 4, 2, 0], [0, 0, 2, 4, 0]) == pytest.approx(4.0, abs=1e-12)
    assert _one([0, 0, 4, 2, 0], [0, 2.5, 4, 2, 0]) == 0.0                            # l and w swapped would overlap here
    assert _one([0, 0, 4, 2, 0], [0, 2.5, 2, 4, 0]) == pytest.approx(2 * 0.5, abs=1e-12)
    a, b = [0, 0, 4, 2, 0], [1, 0.5, 3, 1, 0]                                         # areas 8 and 3, intersection 2.5 x 1 = 2.5
    assert _one(a, b, -1) == pytest.approx(2.5 / (8 + 3 - 2.5), abs=1e-12)
    assert _one(a, b, 0) == pytest.approx(2.5 / 8, abs=1e-12) and _one(a, b, 1) == pytest.approx(2.5 / 3, abs=1e-12)
    assert _one(b, a, 0) == pytest.approx(2.5 / 3, abs=1e-12)                         # criterion 0 divides by the boxes operand
    # a square against its 45-degree copy: the regular octagon, 2 (sqrt 2 - 1) s^2
    s = float(np.float32(3.0))
    assert _one([7, 40, s, s, 0.25], [7, 40, s, s, 0.25 + np.pi / 4]) == pytest.approx(2 * (rt2 - 1) * s * s, rel=1e-6)
    # nested: the inner area, at any yaw
    assert _one([10, 20, 4, 2, 0.3], [10.2, 19.9, 0.5, 0.4, 1.1]) == pytest.approx(0.5 * 0.4, rel=1e-6)
    # a perpendicular cross of two bars of width w: w^2
    assert _one([-5, 60, 6, 0.5, 0.7], [-5, 60, 6, 0.5, 0.7 + np.pi / 2]) == pytest.approx(0.25, rel=1e-6)
    # the sign of ry: a bar at ry = pi / 4 heads towards (+x, -z); a probe square there is inside, its mirror image is not
    bar = [0, 0, 4, 0.2, np.pi / 4]
    assert _one(bar, [1, -1, 0.1, 0.1, 0]) == pytest.approx(0.01, rel=1e-6) and _one(bar, [1, 1, 0.1, 0.1, 0]) == 0.0
    # a pair mirrored through the z axis (x -> -x, yaws kept) changes its value when the yaws differ, and does not when they are equal
    a, b = [0, 30, 4, 1, 0.0], [1.5, 31.0, 4, 1, np.pi / 4]
    assert abs(_one(a, b) - _one([0, 30, 4, 1, 0.0], [-1.5, 31.0, 4, 1, np.pi / 4])) > 0.1
    assert _one(a, [1.5, 31.0, 4, 1, 0.0]) == pytest.approx(_one(a, [-1.5, 31.0, 4, 1, 0.0]), abs=1e-12)
    # 3D: y is the bottom face and -y is up: [y - h, y]
    b7, q7 = np.array([[0, 1.5, 10, 4, 1.5, 2, 0.0]]), np.array([[1, 1.0, 10.5, 4, 1.5, 2, 0.0]])
    ih = 1.0 - 0.0                                                                  # [0, 1.5] against [-0.5, 1.0]
    inc = 3 * 1.5 * ih
    assert rc.judge_3d(b7, q7)[0, 0] == pytest.approx(inc / (12 + 12 - inc), abs=1e-12)
    q7[0, 1] = 0.0                                                                  # [-1.5, 0] touches [0, 1.5]
    assert rc.judge_3d(b7, q7)[0, 0] == 0.0
    q7[0, 1] = 3.0                                                                  # [1.5, 3] touches from below: y + h would overlap here
    assert rc.judge_3d(b7, q7)[0, 0] == 0.0
    assert rc.judge_bev(np.zeros((0, 5)), np.zeros((3, 5))).shape == (0, 3)


def test_band_3d_is_the_exact_effect_of_an_area_excursion():
    rng = np.random.default_rng(0)
    ai, ih, v1, v2, e = rng.uniform(0.1, 5, 50), rng.uniform(0.1, 1.5, 50), rng.uniform(8, 12, 50), rng.uniform(8, 12, 50), 1e-3
    v = lambda a: a * ih / (v1 + v2 - a * ih)
    w = e / (1 + ai)
    bound = rc.band_3d(ai, ih, v1 + v2, w)
    assert np.allclose(v(ai + e) - v(ai), bound, rtol=1e-9) and (np.abs(v(ai - e) - v(ai)) <= bound).all()
    assert rc.band_3d(np.array([1.0]), np.array([0.0]), np.array([20.0]), 1e-3)[0] == 0.0


# ------------------------------------------------------------------------------------------------ the bands
@functools.lru_cache(maxsize=None)
def _measured(name):
    b, q, _, judge = rc.case(name)
    w = p = 0.0
    for c in rc.CRITERIA:
        v = _oracle(b, q, c)
        exc = rc.excursion(v, judge[c], c)
        w, p = max(w, float(exc.max())), max(p, rc.percentile_999(exc[rc.live(v, judge[c])]))
    return w, p


@pytest.mark.parametrize("name", list(rc.GENERATORS) + ["uniform_10"])
def test_bands_are_the_measured_ones(name):
    """W_g and Q_g re-measured on the oracle: measured <= recorded <= 2 x measured (a stale constant cannot hide a loose band), and the
    oracle itself meets both device conditions."""
    w, p = _measured(name)
    rw, rp = rc.BANDS[name]
    print(f"{name}: measured W {w:.4e} Q {p:.4e}, recorded {rw:.3e} {rp:.3e}")
    assert w <= rw <= 2 * w and p <= rp <= 2 * p
    b, q, _, judge = rc.case(name)
    for c in rc.CRITERIA:
        v = _oracle(b, q, c)
        frac, beyond, n = rc.band_report(v, judge[c], c, name)
        assert rc.fits(v, judge[c], c, name) and frac <= 0.25 + 1e-9 and beyond == 0, (c, frac, beyond, n)


# ------------------------------------------------------------------------------------------------ the generators
def test_generator_conditions():
    for name in rc.GENERATORS:
        b, q, area, _ = rc.case(name)
        assert b.shape == q.shape == (rc.N, 5) and b.dtype == q.dtype == np.float32 and np.isfinite(b).all() and np.isfinite(q).all()
        a1, a2 = b[:, 2].astype(np.float64) * b[:, 3], q[:, 2].astype(np.float64) * q[:, 3]
        # both areas positive and different (by 2 % and more for half of the pairs): criterion 0 differs from criterion 1
        assert (a1 > 0).all() and (a2 > 0).all() and (a1 != a2).all() and np.median(np.abs(a1 - a2) / a1) > 0.02, name
        assert np.abs(b[:, 0]).max() < 48 and -8 < b[:, 1].min() and b[:, 1].max() < 88       # KITTI's range
    over = {name: rc.case(name)[2] > 0 for name in rc.GENERATORS}
    for cls in rc.CLASS_SIZE:                      # clusters: the diagonal overlaps (almost all of it) and so do many off-diagonal pairs
        o = over["kitti_jitter_" + cls]
        assert np.diag(o).sum() >= 240 and o.sum() - np.diag(o).sum() >= 1000, cls       # (a 0.6 m wide cyclist moved by sigma 0.3 m can miss)
    assert np.diag(over["near_parallel"]).all() and over["near_parallel"].sum() >= 1500
    for name in ("same_yaw_shifted", "nested", "crossed"):
        assert np.diag(over[name]).all() and over[name].sum() - rc.N < 50, name
    # near_parallel: yaw differs, by a little, never by 0
    b, q, _, _ = rc.case("near_parallel")
    d = np.abs(q[:, 4].astype(np.float64) - b[:, 4])
    assert (d > 5e-6).all() and d.max() < 6e-3
    # same_yaw_shifted: the same yaw bits; no edge line of the query on one of the box
    b, q, _, _ = rc.case("same_yaw_shifted")
    assert np.array_equal(b[:, 4].view(np.int32), q[:, 4].view(np.int32))
    c, s = np.cos(b[:, 4].astype(np.float64)), np.sin(b[:, 4].astype(np.float64))
    dx, dz = q[:, 0].astype(np.float64) - b[:, 0], q[:, 1].astype(np.float64) - b[:, 1]
    du, dv = dx * c - dz * s, dx * s + dz * c
    for shift, k in ((du, 2), (dv, 3)):
        for sign in (-1, 1):                       # the four edge lines per axis: offsets shift +- q/2 against +- b/2
            for side in (-1, 1):
                assert (np.abs(shift + sign * q[:, k] / 2.0 - side * b[:, k] / 2.0) > 0.04).all()
    # nested: the intersection is the smaller box (corners only), in both directions, at least 0.1 m inside
    b, q, area, _ = rc.case("nested")
    a1, a2 = b[:, 2].astype(np.float64) * b[:, 3], q[:, 2].astype(np.float64) * q[:, 3]
    assert np.allclose(np.diag(area), np.minimum(a1, a2), rtol=1e-9) and (a1[0::2] > a2[0::2]).all() and (a1[1::2] < a2[1::2]).all()
    shrunk_b, shrunk_q = b.astype(np.float64), q.astype(np.float64)
    shrunk_b[a1 > a2, 2:4] -= 0.2
    shrunk_q[a2 > a1, 2:4] -= 0.2
    assert np.allclose(np.diag(rc.judge_area(shrunk_b, shrunk_q)), np.minimum(a1, a2), rtol=1e-9)   # still inside the larger box shrunk by 0.1 m per side
    # crossed: the parallelogram of two strips, w1 w2 / sin(difference of yaw): crossings only
    b, q, area, _ = rc.case("crossed")
    dy = q[:, 4].astype(np.float64) - b[:, 4]
    assert (np.abs(np.sin(dy)) >= np.sin(np.deg2rad(60)) - 1e-6).all()
    assert np.allclose(np.diag(area), b[:, 3].astype(np.float64) * q[:, 3] / np.abs(np.sin(dy)), rtol=1e-9)
    # far: every pair more than 1 m apart; the judge and the oracle say exactly 0, with +0.0 bits
    b, q, area, _ = rc.case("far")
    rb, rq = np.hypot(b[:, 2], b[:, 3]) / 2.0, np.hypot(q[:, 2], q[:, 3]) / 2.0
    assert ((q[None, :, 0].astype(np.float64) - b[:, None, 0]) - rb[:, None] - rq[None, :] > 1.0).all() and not area.any()
    for crit in rc.CRITERIA:
        assert not _oracle(b, q, crit).view(np.int32).any()


# ------------------------------------------------------------------------------------------------ the coincident regime
def test_coincident_shares_are_the_recorded_ones():
    """Share of coincident pairs whose oracle IoU is below 0.99 of the true IoU, per sub-case: printed, and equal to what
    rot_eval_contract.COINCIDENT_SHARE records.  No pair exceeds the truth by more than the band, in any sub-case and under any criterion:
    with one shared edge line that is the doing of the on-both-segments test of a crossing (csrc/rot_eval.h, RIE_CROSS_TOL), without
    which 93 of the 257 pairs did (IoU from -34.6 to +30.8, intersection areas up to 672 m2 for cars)."""
    wild = {}
    for sub, recorded in rc.COINCIDENT_SHARE.items():
        b, q, _, judge = rc.case("coincident/" + sub)
        v = _oracle(b, q, -1)
        d, j = np.diag(v).astype(np.float64), np.diag(judge[-1])
        share = float(np.mean(d < 0.99 * j))
        w = rc.BAND_FACTOR * rc.BANDS["kitti_jitter_car"][0]
        wild[sub] = sum(int((_oracle(b, q, c) > judge[c] + w * (1 + judge[c] * (c == 2))).sum()) + int((_oracle(b, q, c) < 0).sum()) for c in rc.CRITERIA)
        print(f"coincident/{sub}: {share:.4f} of {len(d)} pairs below 0.99 of the true IoU; IoU in [{d.min():.4g}, {d.max():.4g}], {wild[sub]} above the truth")
        assert np.isfinite(v).all() and (j > 0.3).all() and round(share, 4) == recorded, sub
        off = v.copy()
        np.fill_diagonal(off, 0)
        assert not off.any()                                                       # the grid: every other pair is disjoint
    assert not any(wild.values()), wild
    b, q, _, judge = rc.case("coincident/identical_yaw0")
    assert np.abs(np.diag(_oracle(b, q, -1)) - 1).max() <= rc.BAND_FACTOR * rc.BANDS["kitti_jitter_car"][0]


# ------------------------------------------------------------------------------------------------ the AP set
def test_ap_set_keeps_clear_of_every_threshold():
    gt, dt = rc.ap_set()
    assert len(gt) == len(dt) == 40 and all(1 <= len(g["name"]) <= 6 and len(d["name"]) == len(g["name"]) + 1 for g, d in zip(gt, dt))
    assert {str(n) for g in gt for n in g["name"]} == set(rc.AP_NAMES)
    assert np.array_equal(rc.ap_min_overlaps(), ke._MIN_OVERLAPS_FULL[:, :, [0, 1, 2]])
    assert set(rc.AP_THRESHOLDS) == set(rc.ap_min_overlaps()[:, 1:].ravel())
    bev, d3, overlapping = rc.ap_margins(gt, dt)
    worst = min(min(float(m.min()) for m in bev), min(float(m.min()) for m in d3))
    print(f"AP set: {overlapping} overlapping pairs, the nearest overlap is {worst:.2e} outside its band around a threshold")
    assert overlapping >= 150 and worst > 0


@functools.lru_cache(maxsize=None)
def _ap_tables(source, metric):
    gt, dt = rc.ap_set()
    rot = rc.judge_bev if source == "judge" else _oracle
    return ke.eval_class(gt, dt, [0, 1, 2], [0, 1, 2], metric, rc.ap_min_overlaps(), rotate_iou=rot)


@pytest.mark.parametrize("metric", [1, 2])
def test_ap_tables_of_the_judge_equal_the_oracles(metric):
    """no tolerance: the fp32 oracle's overlaps give the precision and recall rows of the float64 geometric ones, bit for bit"""
    a, b = _ap_tables("judge", metric), _ap_tables("oracle", metric)
    for key in ("precision", "recall"):
        assert a[key].shape == (3, 3, 2, 41) and a[key].tobytes() == b[key].tobytes(), key
    for c in range(3):
        p = a["precision"][c]
        assert ((p > 0) & (p < 1)).any(), (metric, c)
