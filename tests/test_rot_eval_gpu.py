"""-m gpu: the KITTI rotated-overlap kernels (csrc/rot_eval.h's rie_pair behind md_rotate_iou_eval and behind metrics 1 and 2 of
md_kitti_eval_overlaps) held to the float64 geometric judge and the measured bands of tests/rot_eval_contract.py -- never to the
fp32 oracle's restatement of the same algorithm (except where both sides are exact: yaw 0), never to kitti_eval.calculate_overlaps
(which calls the kernel under test).  The AP tables of both product paths are compared with the judge's without a tolerance.

Worst device excursion as a fraction of the band (4 W_g) per criterion -1 / 0 / 1 / 2, from the first run on an MI355X; no live pair
of any generator was beyond 4 Q_g (0.25 is the oracle's own worst by construction: the device then has the oracle's value there):
    kitti_jitter_car          0.249  0.153  0.145  0.143      (1815 live pairs)
    kitti_jitter_pedestrian   0.248  0.143  0.139  0.047      (2017)
    kitti_jitter_cyclist      0.300  0.226  0.211  0.145      (1344)
    near_parallel             0.248  0.161  0.160  0.157      (1677)
    same_yaw_shifted          0.190  0.178  0.198  0.250      (293)
    nested                    0.018  0.218  0.249  0.071      (257)
    crossed                   0.119  0.216  0.227  0.249      (257)
    far                       all bits zero
    md_kitti_eval_overlaps    metric 1: 0.053, metric 2: 0.037 of the band (195 / 192 live pairs, none beyond 4 Q)
    uniform_10 (tests/test_nms_iou_gpu.py::test_rotate_iou_eval_vs_oracle)   0.116  0.319  0.167  0.330      (2653)
    coincident, share of pairs below 0.99 of the true IoU: identical 0.9883, identical_quarter 0.7471, identical_yaw0 0 (all three the
    oracle's shares), shared_edge 0.1362 (the oracle's too); no value of any sub-case below 0 or above judge + 4 W
The AP tables of the host path and of the device backend were bit-equal to the judge's for metrics 1 and 2.
Before rie_pair kept a crossing only if it lies on both segments (csrc/rot_eval.h, RIE_CROSS_TOL), the shared_edge sub-case failed
its range condition on the device as on the oracle: see test_coincident_pairs_stay_finite_and_lose_area_only.  Every other figure
above was the same before and after.
"""
import functools

import numpy as np
import pytest
import torch

import oracle
from tests import rot_eval_contract as rc
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]

DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # a copy: the contract's shared cases are read-only


def _device(b, q, criterion):
    from minddet_amd import det_ops
    return det_ops.rotate_iou_gpu_eval(T(b), T(q), criterion).cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


# ------------------------------------------------------------------------------------------------ 1: md_rotate_iou_eval against the judge
@pytest.mark.parametrize("name", list(rc.GENERATORS))
def test_rotate_iou_eval_fits_the_judges_band(name):
    """every criterion: all pairs within 4 W_g of the judge, at most 1 live pair in 1000 beyond 4 Q_g; `far`: all bits zero"""
    b, q, _, judge = rc.case(name)
    report = []
    for c in rc.CRITERIA:
        v = _device(b, q, c)
        assert v.shape == judge[c].shape and v.dtype == np.float32
        report.append((c, v) + rc.band_report(v, judge[c], c, name))
    print(f"{name}: " + "; ".join(f"criterion {c}: {frac:.3f} of the band, {beyond} of {n} live pairs beyond 4 Q" for c, _, frac, beyond, n in report))
    for c, v, frac, beyond, n in report:
        if name == "far":
            assert not _bits(v).any(), c
        assert rc.fits(v, judge[c], c, name), (name, c, frac, beyond, n)


# ------------------------------------------------------------------------------------------------ 2: the operands
@pytest.mark.parametrize("name", ["kitti_jitter_car", "nested"])
def test_the_operands_are_not_interchangeable(name):
    b, q, _, judge = rc.case(name)
    c0, c1, swapped = _device(b, q, 0), _device(b, q, 1), _device(q, b, 1)
    assert np.array_equal(_bits(c0), _bits(swapped.T))              # criterion 0 divides by the boxes operand, 1 by the query operand
    on = judge[-1] > 0
    assert on.sum() >= rc.N and (c0[on] != c1[on]).all()


# ------------------------------------------------------------------------------------------------ 3: md_kitti_eval_overlaps
@functools.lru_cache(maxsize=None)
def _overlap_images():
    """the AP set, then blocks with G = 0, D = 0, both, 65 x 3 and 3 x 70 (both extents across the wave width), then an image whose
    detections overlap its first ground truth in BEV while their height intervals touch it exactly (from above and from below), are
    disjoint from it, and overlap it"""
    gt, dt = (list(a) for a in rc.ap_set())
    rng = np.random.default_rng(11)
    for D, G in ((0, 3), (4, 0), (0, 0), (65, 3), (3, 70)):
        g = rc.objects(rng, [rc.AP_NAMES[k] for k in rng.integers(0, 3, G)])
        k = min(D, G)
        gt.append(g)
        dt.append(rc.detections_on(rng, g, k, [rc.AP_NAMES[j] for j in rng.integers(0, 3, D - k)]))
    g = rc.objects(rng, ["Car", "Pedestrian"])
    g["location"][0, 1], g["dimensions"][0, 1] = 1.5, 1.5            # the first ground truth spans [0, 1.5]; every number below is exact
    d = rc.detections_on(rng, {k: np.repeat(v[:1], 4, 0) for k, v in g.items()}, 4, [])
    d["location"][0, 1], d["dimensions"][0, 1] = 0.0, 2.0            # [-2, 0]: touches from above (-y is up); [y, y + h] would overlap by 0.5
    d["location"][1, 1], d["dimensions"][1, 1] = 3.0, 1.5            # [1.5, 3]: touches from below
    d["location"][2, 1], d["dimensions"][2, 1] = -0.5, 1.25          # [-1.75, -0.5]: disjoint
    gt.append(g)
    dt.append(d)
    return gt, dt


def test_kitti_eval_overlaps_fit_the_judges_band():
    from minddet_amd import det_ops
    from minddet_amd import kitti_eval as ke
    gt, dt = _overlap_images()
    p = ke.pack_annos(gt, dt, device=DEV)
    o_off = p.ov_off.cpu().numpy()
    assert p.pairs == o_off[-1] == sum(len(g["name"]) * len(d["name"]) for g, d in zip(gt, dt))
    q = {n: rc.BANDS["kitti_jitter_" + n.lower()][1] for n in rc.AP_NAMES}
    for metric in (1, 2):
        got = det_ops.kitti_eval_overlaps(p.gt_off, p.dt_off, p.ov_off, p.gt_cam, p.dt_cam, metric, p.pairs).cpu().numpy()
        worst, beyond, live, zero_height = 0.0, 0, 0, 0
        for i, (g, d) in enumerate(zip(gt, dt)):
            G, D = len(g["name"]), len(d["name"])
            block = got[o_off[i]:o_off[i + 1]].reshape(G, D).T             # [D, G]: the detection is the boxes operand
            if block.size == 0:
                continue
            cd, cg = rc.cam_boxes(d), rc.cam_boxes(g)
            w = rc.BAND_FACTOR * rc.ap_band_w(d["name"], g["name"])
            wq = rc.BAND_FACTOR * np.maximum(np.array([q[str(n)] for n in d["name"]])[:, None], np.array([q[str(n)] for n in g["name"]])[None, :])
            if metric == 1:
                want = rc.judge_bev(cd[:, [0, 2, 3, 5, 6]], cg[:, [0, 2, 3, 5, 6]], -1)
                band, band_q = w, wq
            else:
                want, ai, ih, vsum = rc.judge_3d(cd, cg, parts=True)
                band, band_q = rc.band_3d(ai, ih, vsum, w), rc.band_3d(ai, ih, vsum, wq)
                flat = (ai > 0) & (ih <= 0)
                zero_height += int(flat.sum())
                assert not _bits(block[flat]).any(), i                       # touching or disjoint heights over a BEV overlap: exactly 0
            assert np.isfinite(block).all()
            exc = np.abs(block - want)
            with np.errstate(all="ignore"):
                worst = max(worst, float(np.where(band > 0, exc / band, np.where(exc > 0, np.inf, 0.0)).max()))
            lv = (want > 0) | (block != 0)
            beyond += int((exc[lv] > band_q[lv]).sum())
            live += int(lv.sum())
            assert (exc <= band).all(), (metric, i, float(exc.max()))
        print(f"md_kitti_eval_overlaps metric {metric}: worst excursion {worst:.3f} of the band, {beyond} of {live} live pairs beyond 4 Q")
        assert beyond * 1000 <= live and live >= 180
        assert metric == 1 or zero_height >= 3


# ------------------------------------------------------------------------------------------------ 4: AP without a tolerance
@functools.lru_cache(maxsize=None)
def _tables(source, metric):
    """(precision, recall, the per-threshold (tp, fp, fn) tables in (class, difficulty, level) order) on the AP set: source "judge" =
    eval_class on the float64 geometric overlaps, "host" = eval_class on its product overlap source (md_rotate_iou_eval per image),
    "device" = eval_class_device"""
    from minddet_amd import kitti_eval as ke
    gt, dt = rc.ap_set()
    counts = []
    tail = ke._curves_from_counts

    def spy(pr, *rest):
        counts.append(np.array(pr[:, :3]))
        return tail(pr, *rest)
    ke._curves_from_counts = spy
    try:
        if source == "device":
            ret = ke.eval_class_device(ke.pack_annos(gt, dt, device=DEV), [0, 1, 2], [0, 1, 2], metric, rc.ap_min_overlaps())
        else:
            ret = ke.eval_class(gt, dt, [0, 1, 2], [0, 1, 2], metric, rc.ap_min_overlaps(), rotate_iou=rc.judge_bev if source == "judge" else None)
    finally:
        ke._curves_from_counts = tail
    return ret["precision"], ret["recall"], counts


@pytest.mark.parametrize("metric", [1, 2])
@pytest.mark.parametrize("source", ["host", "device"])
def test_ap_tables_are_the_judges(source, metric):
    """three classes, three difficulties, both overlap levels: precision, recall and the tp / fp / fn counts per threshold, bit for bit"""
    precision, recall, counts = _tables(source, metric)
    want_p, want_r, want_c = _tables("judge", metric)
    assert precision.shape == want_p.shape == (3, 3, 2, 41) and len(counts) == len(want_c) == 18
    assert precision.tobytes() == want_p.tobytes() and recall.tobytes() == want_r.tobytes()
    for a, b in zip(counts, want_c):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert all(((want_p[c] > 0) & (want_p[c] < 1)).any() for c in range(3)) and max(len(c) for c in want_c) >= 10


# ------------------------------------------------------------------------------------------------ 5: the coincident regime
@pytest.mark.parametrize("sub", list(rc.COINCIDENT_SHARE))
def test_coincident_pairs_stay_finite_and_lose_area_only(sub):
    """every value finite and in [0, judge + 4 W] (criterion 2: judge + 4 W (1 + judge)), W the cars'; yaw exactly 0: bit-equal to the
    oracle (the trig is exact on both sides) and within the band of 1.  The share of pairs below 0.99 of the truth is printed, not
    compared with the oracle's: one last bit of cosf flips the non-strict corner test.

    [shared_edge] is what the on-both-segments test of a crossing is for (csrc/rot_eval.h, RIE_CROSS_TOL): without it two collinear edges
    gave a "crossing" that was a quotient of two rounding residues.  MI355X before it, 257 pairs: criterion -1 in [-34.55, 11.14] with 29
    values above judge + 4 W, criteria 0 / 1 / 2 up to 97.56 / 188.0 / 671.5 (m2, for 6 m2 cars) with 97 values above."""
    b, q, _, judge = rc.case("coincident/" + sub)
    w = rc.BAND_FACTOR * rc.BANDS["kitti_jitter_car"][0]
    out = {c: _device(b, q, c) for c in rc.CRITERIA}
    d, j = np.diag(out[-1]).astype(np.float64), np.diag(judge[-1])
    print(f"coincident/{sub}: {np.mean(d < 0.99 * j):.4f} of {len(d)} pairs below 0.99 of the true IoU (oracle: {rc.COINCIDENT_SHARE[sub]:.4f}); "
          + "; ".join(f"criterion {c}: values in [{out[c].min():.4g}, {out[c].max():.4g}], {int((out[c] > judge[c] + w * (1 + judge[c] * (c == 2))).sum())} above the truth"
                      for c in rc.CRITERIA))
    if sub == "identical_yaw0":
        for c in rc.CRITERIA:
            assert np.array_equal(_bits(out[c]), _bits(oracle.rotate_iou_eval(b, q, c))), c
        assert np.abs(d - 1).max() <= w
    for c in rc.CRITERIA:
        v = out[c].astype(np.float64)
        assert np.isfinite(v).all() and (v >= 0).all(), (sub, c, float(v.min()))
        assert (v <= judge[c] + w * (1 + judge[c] * (c == 2))).all(), (sub, c, float((v - judge[c]).max()))


# ------------------------------------------------------------------------------------------------ 6: launch shape
GUARD = 256


def _launch(b, q, criterion, stream=None):
    """md_rotate_iou_eval on an output in the middle of a buffer pre-filled with 0x5a bytes; returns the buffer, not synchronised"""
    from minddet_amd import _lib, det_ops
    n, k = b.shape[0], q.shape[0]
    buf = torch.full(((n * k + 2 * GUARD) * 4,), 0x5A, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()                                          # the fill is done before another stream writes into it
    out = buf.view(torch.float32)[GUARD:GUARD + n * k].view(n, k)
    _lib.call("md_rotate_iou_eval", [b, q, out], extra=det_ops._RotIouAttrs(int(criterion)), stream=stream)
    return buf


def _parts(buf, cells):
    """(front guard, output, back guard) bytes of a _launch buffer"""
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    return raw[:GUARD * 4], raw[GUARD * 4:(GUARD + cells) * 4], raw[(GUARD + cells) * 4:]


@pytest.mark.parametrize("n,k", [(1, 1), (1, 257), (257, 1), (255, 3)])
def test_launch_shapes_write_every_element_and_nothing_else(n, k):
    b, q, _, judge = rc.case("kitti_jitter_car")
    rows = np.arange(n) if n > 1 else np.array([5])
    cols = np.arange(k) if k > 1 else np.array([5])
    if (n, k) == (255, 3):
        cols = np.array([0, 1, 254])                                  # the diagonal pairs (0, 0), (1, 1), (254, 254) overlap
    tb, tq = T(b[rows]), T(q[cols])
    front, body, back = _parts(_launch(tb, tq, -1), n * k)
    assert (front == 0x5A).all() and (back == 0x5A).all()
    v = body.view(np.float32).reshape(n, k)
    assert not (body.view(np.uint32) == 0x5A5A5A5A).any()             # 1.5e16 is no IoU: every element was written
    want = judge[-1][np.ix_(rows, cols)]
    assert (rc.excursion(v, want, -1) <= rc.BAND_FACTOR * rc.BANDS["kitti_jitter_car"][0]).all() and (want > 0).any()
    assert _parts(_launch(tb, tq, -1), n * k)[1].tobytes() == body.tobytes()        # two calls: identical bytes
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    bufs = [_launch(tb, tq, -1, stream=s.cuda_stream) for s in streams]              # both in flight, then one synchronisation
    for buf in bufs:                                                  # two streams agree, with each other and with the first call
        f, v2, t = _parts(buf, n * k)
        assert v2.tobytes() == body.tobytes() and (f == 0x5A).all() and (t == 0x5A).all()
