"""-m gpu: the KITTI AP evaluation on the device (include/minddet_hip_kittieval.h) judged by the host evaluator it replaces
(minddet_amd/kitti_eval.py) and by the reference's recorded outputs (tests/golden/kitti_eval_vectors.json) -- never by itself.
Flags, overlaps, matched scores, thresholds and the per-image counts are compared exactly; the precision rows of the fixture at the
host path's own 1e-12; the AOS sums within a bound stated in test_aos_sum_within_the_stated_bound."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
MO_MS = np.array([[[0.7, 0.5, 0.5]] * 3, [[0.5, 0.25, 0.25]] * 3])


def _np_anno(a):
    return {k: (np.array(v) if k == "name" else np.asarray(v, float if k != "occluded" else int)) for k, v in a.items()}


@functools.lru_cache(maxsize=None)
def _golden_cases():
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "kitti_eval_vectors.json")))
    return [([_np_anno(a) for a in c["gt"]], [_np_anno(a) for a in c["dt"]], c) for c in gold["cases"]]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ----------------------------------------------------------------------------- 1: flags
@pytest.mark.parametrize("table", ["full", "ms"])
def test_flags_equal_clean_data(table):
    from minddet_amd import det_ops
    from minddet_amd import kitti_eval as ke
    names = ke.CLASS_NAMES_MS if table == "ms" else ke.CLASS_NAMES_FULL
    gt, dt, _ = _golden_cases()[0]
    gt = [dict(a) for a in gt]
    i0, j0 = next((i, j) for i, a in enumerate(gt) for j, n in enumerate(a["name"]) if n == "Car" and a["occluded"][j] <= 2 and a["truncated"][j] <= 0.5)
    box = gt[i0]["bbox"].reshape(-1, 4).copy()
    box[j0, [1, 3]] = box[j0, [3, 1]] + [60.0, 0.0]                  # a negative height of 60 px or more: counted by the "ms" table, ignored by the full one
    gt[i0]["bbox"] = box
    assert box[j0, 3] - box[j0, 1] <= -60
    p = ke.pack_annos(gt, dt, names, device=DEV)
    ign_gt, ign_dt, num_valid = det_ops.kitti_eval_flags(p.gt_box, p.gt_occ, p.gt_trunc, p.gt_valid, p.dt_box, p.dt_same, p.abs_gt_height)
    ign_gt, ign_dt, num_valid = ign_gt.cpu().numpy().astype(int) - 1, ign_dt.cpu().numpy().astype(int) - 1, num_valid.cpu().numpy()
    g_off, d_off = p.gt_off.cpu().numpy(), p.dt_off.cpu().numpy()
    for c in range(len(names)):
        for d in range(3):
            total = 0
            for i, (g, t) in enumerate(zip(gt, dt)):
                nv, ig, idt, _ = ke.clean_data(g, t, c, d, names)
                total += nv
                assert ign_gt[c, d, g_off[i]:g_off[i + 1]].tolist() == list(ig), (c, d, i)
                assert ign_dt[c, d, d_off[i]:d_off[i + 1]].tolist() == list(idt), (c, d, i)
            assert num_valid[c, d] == total
    assert ign_gt[0, 2, g_off[i0] + j0] == (0 if table == "ms" else 1) and num_valid[0, 2] > 0 and (ign_dt == 1).any() and (ign_gt == -1).any()


# ----------------------------------------------------------------------------- 2: overlaps
def _boxes(rng, n, with_score):
    """tests/test_kitti_eval_gpu.py's cars for a given count (0 gives the empty annotation's shapes)"""
    loc = np.stack([rng.uniform(-15, 15, n), np.full(n, 1.6), rng.uniform(5, 45, n)], 1)
    dims = np.stack([rng.uniform(3.2, 4.6, n), rng.uniform(1.4, 1.7, n), rng.uniform(1.5, 1.8, n)], 1)
    u = 600 + 700 * loc[:, 0] / loc[:, 2]
    half = 700 * 2.0 / loc[:, 2]
    bbox = np.stack([u - half, 180 - 40 - 600 / loc[:, 2], u + half, 180 + 600 / loc[:, 2]], 1)
    a = dict(name=np.array(["Car"] * n), bbox=bbox, location=loc, dimensions=dims, rotation_y=rng.uniform(-3, 3, n),
             occluded=rng.integers(0, 3, n), truncated=rng.choice([0.0, 0.2, 0.4], n), alpha=rng.uniform(-3, 3, n))
    if with_score:
        a["score"] = rng.uniform(0.1, 1.0, n)
    return a


@functools.lru_cache(maxsize=None)
def _seeded_24():
    """the 24 images of tests/test_kitti_eval_gpu.py, by its generator and in its order of draws"""
    from tests.test_kitti_eval_gpu import _annos
    rng = np.random.default_rng(5)
    gt = _annos(rng, 24, False)
    dt = []
    for g in gt:
        d = {k: np.array(v) for k, v in g.items()}
        d["location"] = d["location"] + rng.normal(0, 0.15, d["location"].shape)
        d["rotation_y"] = d["rotation_y"] + rng.normal(0, 0.05, d["rotation_y"].shape)
        d["score"] = rng.uniform(0.1, 1.0, len(d["name"]))
        dt.append(d)
    return gt, dt


def test_overlaps_are_bit_equal_to_the_host_blocks():
    from minddet_amd import det_ops
    from minddet_amd import kitti_eval as ke
    gt, dt = (list(a) for a in _seeded_24())
    rng = np.random.default_rng(11)
    for D, G in ((0, 3), (4, 0), (0, 0), (65, 3), (3, 70)):          # empty blocks; both extents across the wave width
        g = _boxes(rng, G, False)
        d = _boxes(rng, D, True)
        k = min(D, G)
        if k:                                                        # some detections lie on a ground truth
            for key in ("location", "dimensions"):
                d[key][:k] = g[key][:k] + rng.normal(0, 0.1, (k, 3))
            d["rotation_y"][:k] = g["rotation_y"][:k] + rng.normal(0, 0.05, k)
            d["bbox"][:k] = g["bbox"][:k] + rng.normal(0, 2.0, (k, 4))
        gt.append(g)
        dt.append(d)
    p = ke.pack_annos(gt, dt, device=DEV)
    o_off = p.ov_off.cpu().numpy()
    assert p.pairs == o_off[-1] == sum(len(g["name"]) * len(d["name"]) for g, d in zip(gt, dt))
    for metric in (0, 1, 2):
        got = det_ops.kitti_eval_overlaps(p.gt_off, p.dt_off, p.ov_off, *((p.gt_box, p.dt_box) if metric == 0 else (p.gt_cam, p.dt_cam)), metric, p.pairs)
        got = got.cpu().numpy()
        want = ke.calculate_overlaps(gt, dt, metric)                 # metrics 1 and 2: md_rotate_iou_eval per image, so equality shows the shared pair arithmetic
        nonzero = 0
        for i, w in enumerate(want):
            G, D = len(gt[i]["name"]), len(dt[i]["name"])
            assert w.shape == (D, G)
            block = got[o_off[i]:o_off[i + 1]].reshape(G, D)
            assert np.array_equal(_bits(block.T), _bits(w)), (metric, i, np.abs(block.T - w).max() if w.size else 0)
            nonzero += int((w > 0).sum())
        assert nonzero > 40
    # a longer result than ov_off[I]: the tail is zero
    got = det_ops.kitti_eval_overlaps(p.gt_off, p.dt_off, p.ov_off, p.gt_box, p.dt_box, 0, p.pairs + 300).cpu().numpy()
    assert not got[p.pairs:].any() and got[:p.pairs].any()


# ----------------------------------------------------------------------------- 3, 4: matching, thresholds, counts
MIN_OV = (0.45, 0.25)


@functools.lru_cache(maxsize=None)
def _match_images():
    """the twelve seeded cases of tests/test_kitti_eval_cpu.py::test_matching_equals_the_sequential_scan (the same draws in the same
    order) as twelve images, and a thirteenth with D = 130, G = 70 whose equal top scores sit at detections 3 and 67.  Flags for the
    second and third difficulty come from a generator of their own.  The DontCare boxes of a case are appended as ground-truth rows of
    flag -1 (zero overlaps), which no rule of compute_statistics looks at."""
    imgs = []
    for seed in range(13):
        rng = np.random.default_rng(seed)
        if seed < 12:
            D, G, C = int(rng.integers(0, 14)), int(rng.integers(0, 9)), int(rng.integers(0, 3))
        else:
            D, G, C = 130, 70, 2
        overlaps = np.round(rng.random((D, G)), 1)
        gt = np.concatenate([rng.random((G, 4)) * 100, rng.uniform(-3, 3, (G, 1))], 1)
        dt = np.concatenate([np.sort(rng.random((D, 4)) * 300, 1)[:, [0, 1, 2, 3]], rng.uniform(-3, 3, (D, 1)), np.round(rng.random((D, 1)), 1)], 1)
        dt[:, :4] = dt[:, [0, 1, 2, 3]]
        ig, idt = rng.integers(-1, 2, G), rng.integers(-1, 2, D)
        dc = np.sort(rng.random((C, 4)) * 300, 1)
        more = np.random.default_rng(100 + seed)
        igs, idts = [ig, more.integers(-1, 2, G), more.integers(-1, 2, G)], [idt, more.integers(-1, 2, D), more.integers(-1, 2, D)]
        if seed == 12:
            overlaps[:, 0] = 0.1
            overlaps[[3, 67], 0] = 0.9
            overlaps[[3, 67], 1] = 0.8                                # the second ground truth can only take the one the first left
            dt[:, 5] = np.minimum(dt[:, 5], 0.9)
            dt[[3, 67], 5] = 0.95
            for d in range(3):
                igs[d][:2] = 0
                idts[d][[3, 67]] = 0
        imgs.append(dict(D=D, G=G, C=C, ov=overlaps, gt=gt, dt=dt, ig=igs, idt=idts, dc=dc))
    return imgs


@functools.lru_cache(maxsize=None)
def _match_operands():
    """the thirteen images as the operands of md_kitti_eval_match / _stats: one class, three difficulties, two overlap levels"""
    imgs = _match_images()
    Gs = [m["G"] + m["C"] for m in imgs]
    Ds = [m["D"] for m in imgs]
    g_off, d_off = np.concatenate([[0], np.cumsum(Gs)]), np.concatenate([[0], np.cumsum(Ds)])
    o_off = np.concatenate([[0], np.cumsum(np.array(Gs) * np.array(Ds))])
    ov = np.concatenate([np.concatenate([m["ov"].T, np.zeros((m["C"], m["D"]))], 0).reshape(-1) for m in imgs])
    ign_gt = np.stack([np.concatenate([np.concatenate([m["ig"][d], np.full(m["C"], -1)]) for m in imgs]) for d in range(3)])[None] + 1
    ign_dt = np.stack([np.concatenate([m["idt"][d] for m in imgs]) for d in range(3)])[None] + 1
    t = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)
    ops = dict(ov=t(ov, np.float64), ign_gt=t(ign_gt, np.uint8), ign_dt=t(ign_dt, np.uint8), dt_score=t(np.concatenate([m["dt"][:, 5] for m in imgs]), np.float64),
               gt_off=t(g_off, np.int32), dt_off=t(d_off, np.int32), ov_off=t(o_off, np.int64), min_overlap=t(np.array([MIN_OV]), np.float64),
               gt_box=t(np.concatenate([np.concatenate([m["gt"][:, :4], m["dc"]], 0) for m in imgs]), np.float64),
               gt_dc=t(np.concatenate([np.concatenate([np.zeros(m["G"]), np.ones(m["C"])]) for m in imgs]), np.uint8),
               dt_box=t(np.concatenate([m["dt"][:, :4] for m in imgs]), np.float64),
               gt_alpha=t(np.concatenate([np.concatenate([m["gt"][:, 4], np.zeros(m["C"])]) for m in imgs]), np.float64),
               dt_alpha=t(np.concatenate([m["dt"][:, 4] for m in imgs]), np.float64))
    ops["num_valid"] = t(_num_valid(), np.int32)
    return ops, g_off


def _num_valid():
    return np.array([[sum(int((m["ig"][d] == 0).sum()) for m in _match_images()) for d in range(3)]])


def _first(ops):
    return [ops[k] for k in ("ov", "ign_gt", "ign_dt", "dt_score", "gt_off", "dt_off", "ov_off", "min_overlap")]


@functools.lru_cache(maxsize=None)
def _host_pass1():
    """per (difficulty, level): the matched scores of each image by compute_statistics, and get_thresholds of all of them"""
    from minddet_amd import kitti_eval as ke
    imgs = _match_images()
    num_valid = _num_valid()
    out = {}
    for d in range(3):
        for k, mo in enumerate(MIN_OV):
            scores = [ke.compute_statistics(m["ov"], m["gt"], m["dt"], m["ig"][d], m["idt"][d], m["dc"], 0, mo, 0.0, False)[4] for m in imgs]
            out[d, k] = (scores, ke.get_thresholds(np.concatenate(scores), int(num_valid[0, d])))
    return out


def test_match_and_thresholds_equal_the_host():
    from minddet_amd import det_ops
    imgs = _match_images()
    ops, g_off = _match_operands()
    matched = det_ops.kitti_eval_match(*_first(ops))
    thresholds, nthresh = det_ops.kitti_eval_thresholds(torch.sort(matched, dim=-1, descending=True).values, ops["num_valid"])
    matched, thresholds, nthresh = matched.cpu().numpy(), thresholds.cpu().numpy(), nthresh.cpu().numpy()
    assert matched.shape == (1, 3, 2, g_off[-1]) and thresholds.shape == (1, 3, 2, 41)
    host = _host_pass1()
    for (d, k), (scores, thr) in host.items():
        for i, m in enumerate(imgs):
            row = matched[0, d, k, g_off[i]:g_off[i + 1]]
            assert np.isneginf(row[~np.isfinite(row)]).all()
            assert row[np.isfinite(row)].tolist() == scores[i].tolist(), (d, k, i)
        assert nthresh[0, d, k] == len(thr) > 0 and thresholds[0, d, k, :len(thr)].tolist() == thr, (d, k)
        assert np.isnan(thresholds[0, d, k, len(thr):]).all()
    # the thirteenth image: of the two equal top scores the lower index took the first ground truth, across lane chunks
    m = imgs[12]
    assert matched[0, 0, 0, g_off[12]] == 0.95 == matched[0, 0, 0, g_off[12] + 1] and m["dt"][3, 5] == m["dt"][67, 5] == 0.95
    assert max(len(t) for _, t in host.values()) >= 10


@pytest.mark.parametrize("metric", [0, 1])
def test_stats_equal_compute_statistics(metric):
    from minddet_amd import det_ops
    from minddet_amd import kitti_eval as ke
    imgs = _match_images()
    ops, g_off = _match_operands()
    host = _host_pass1()
    thr = np.full((1, 3, 2, 41), np.nan)
    nth = np.zeros((1, 3, 2), np.int32)
    for (d, k), (_, t) in host.items():
        thr[0, d, k, :len(t)], nth[0, d, k] = t, len(t)
    rest = [torch.from_numpy(thr).to(DEV), torch.from_numpy(nth).to(DEV)] + [ops[k] for k in ("gt_box", "gt_dc", "dt_box", "gt_alpha", "dt_alpha")]
    a = [t.cpu().numpy() for t in det_ops.kitti_eval_stats(*_first(ops), *rest, metric, True)]
    b = [t.cpu().numpy() for t in det_ops.kitti_eval_stats(*_first(ops), *rest, metric, True)]
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()                             # two calls: the same bits, img_sim and pr_sim included
    img_counts, img_sim, pr_counts, pr_sim = a
    assert img_counts.shape == (1, 3, 2, 41, 13, 3) and img_sim.shape == (1, 3, 2, 41, 13) and pr_counts.shape == (1, 3, 2, 41, 3)
    discounted = 0
    for (d, k), (_, t) in host.items():
        for ti, thresh in enumerate(t):
            for i, m in enumerate(imgs):
                tp, fp, fn, sim, _ = ke.compute_statistics(m["ov"], m["gt"], m["dt"], m["ig"][d], m["idt"][d], m["dc"], metric, MIN_OV[k], thresh, True, True)
                assert img_counts[0, d, k, ti, i].tolist() == [tp, fp, fn], (d, k, ti, i)
                assert abs(img_sim[0, d, k, ti, i] - (0.0 if sim == -1 else sim)) <= 1e-12 * max(tp, 1)
                if metric == 0:
                    discounted += fp != ke.compute_statistics(m["ov"], m["gt"], m["dt"], m["ig"][d], m["idt"][d], m["dc"], 1, MIN_OV[k], thresh, True)[1]
        assert np.array_equal(pr_counts[0, d, k], img_counts[0, d, k].sum(1))
        assert not img_counts[0, d, k, len(t):].any() and not img_sim[0, d, k, len(t):].any() and not pr_counts[0, d, k, len(t):].any() and not pr_sim[0, d, k, len(t):].any()
    assert pr_counts[..., 0].max() > 5 and pr_counts[..., 1].max() > 5 and pr_counts[..., 2].max() > 5
    assert metric != 0 or discounted > 0                              # the DontCare discount was exercised


# ----------------------------------------------------------------------------- 5: the reference's own outputs
@pytest.mark.parametrize("c", (0, 1, 2))
def test_fixture_rows_and_text_equal_the_references(c):
    from minddet_amd import kitti_eval as ke
    gt, dt, case = _golden_cases()[c]
    p = ke.pack_annos(gt, dt, ke.CLASS_NAMES_MS, device=DEV)
    ret = ke.eval_class_device(p, [0, 1, 2], [0, 1, 2], 0, MO_MS)
    np.testing.assert_allclose(np.nan_to_num(ret["precision"], nan=-1.0), np.array(case["precision"]), rtol=0, atol=1e-12)
    text, m = ke.get_official_eval_result(gt, dt, [0, 1, 2], protocol="ms", backend="device")
    assert text == case["text"]
    np.testing.assert_allclose(m, np.array(case["map_bbox"]), rtol=0, atol=1e-9)


# ----------------------------------------------------------------------------- 6: the full protocol
def test_full_protocol_equals_the_host_evaluator():
    from minddet_amd import kitti_eval as ke
    gt, dt = _seeded_24()
    mo = ke._MIN_OVERLAPS_FULL[:, :, [0]]
    p = ke.pack_annos(gt, dt, device=DEV)
    for metric in (0, 1, 2):
        dev = ke.eval_class_device(p, [0], [0, 1, 2], metric, mo)
        ref = ke.eval_class(gt, dt, [0], [0, 1, 2], metric, mo)
        assert np.array_equal(dev["precision"], ref["precision"], equal_nan=True), metric
        assert np.array_equal(dev["recall"], ref["recall"], equal_nan=True), metric
        assert dev["precision"].shape == (1, 3, 2, 41) and np.nanmax(dev["precision"]) > 0.5
    text, out = ke.get_official_eval_result(gt, dt, ["Car"], backend="device")
    assert "bev AP:" in text and "aos AP:" in text and "Car_3d/moderate_R40" in out and "Car_aos/easy_R40" in out
    ref_text, ref_out = ke.get_official_eval_result(gt, dt, ["Car"])
    assert set(out) == set(ref_out)
    for k in out:
        assert out[k] == ref_out[k] or ("aos" in k and abs(out[k] - ref_out[k]) <= 1e-10), k


def test_empty_sets_give_the_hosts_rows():
    """no image at all, images without a detection, images without a ground truth: the same code, the host's rows"""
    from minddet_amd import kitti_eval as ke
    gt, dt = _seeded_24()
    mo = ke._MIN_OVERLAPS_FULL[:, :, [0]]
    none = lambda annos, score: [_boxes(np.random.default_rng(0), 0, score) for _ in annos]
    for g, d in (([], []), (gt[:5], none(gt[:5], True)), (none(dt[:5], False), dt[:5])):
        p = ke.pack_annos(g, d, device=DEV)
        for metric in (0, 2):
            dev = ke.eval_class_device(p, [0], [0, 1, 2], metric, mo, compute_aos=metric == 0)
            ref = ke.eval_class(g, d, [0], [0, 1, 2], metric, mo, compute_aos=metric == 0)
            for key in ("precision", "recall", "orientation"):
                assert np.array_equal(dev[key], ref[key], equal_nan=True), (len(g), metric, key)


# ----------------------------------------------------------------------------- 7: AOS
ULP1 = 2.0 ** -52
# Part (b): the worst difference between the device's (1 + cos(delta)) / 2 and numpy's on the single-true-positive images of this test,
# measured on an MI355X over its 6 156 such cells (DESIGN 9 item 20 records it): 1.110e-16 = 2^-53, half an ulp of 1.0.  Twice that is
# allowed per term, and never more than 4 ulp of 1.0.
MEASURED_TERM = 2.0 ** -53
TERM = min(2 * MEASURED_TERM, 4 * ULP1)


def test_aos_sum_within_the_stated_bound():
    """pr_sim against the host's sequential sum.  (a) derived: a float64 sum of N terms in [0, 1] taken in any order differs from the
    exact sum S by at most (N - 1) 2^-53 S to first order, so two orders differ by at most twice that.  (b) per term the device's float64
    cos and numpy's, neither correctly rounded, may differ: TERM above, from a measurement this test repeats and prints."""
    from minddet_amd import kitti_eval as ke
    rng = np.random.default_rng(23)
    N = 300
    gt, dt = [], []
    for i in range(N):                                                # one tall car and one detection on it: a single true positive per image
        box = np.array([[100.0, 100.0, 200.0, 200.0]]) + rng.uniform(-5, 5, (1, 4))
        gt.append(dict(name=np.array(["Car"]), bbox=box, alpha=rng.uniform(-np.pi, np.pi, 1), occluded=np.zeros(1, int), truncated=np.zeros(1)))
        dt.append(dict(name=np.array(["Car"]), bbox=box + rng.uniform(-1, 1, (1, 4)), alpha=rng.uniform(-np.pi, np.pi, 1), score=rng.uniform(0.1, 1.0, 1)))
    mo = np.full((1, 3, 1), 0.7)
    p = ke.pack_annos(gt, dt, device=DEV)
    t = ke.device_tables(p, [0], 0, mo, compute_aos=True)
    nth = int(t["nthresh"][0, 0, 0])
    img_counts, img_sim, pr_sim = t["img_counts"][0, 0, 0].cpu().numpy(), t["img_sim"][0, 0, 0].cpu().numpy(), t["pr_sim"][0, 0, 0].cpu().numpy()
    thr = t["thresholds"][0, 0, 0].cpu().numpy()
    assert nth == 41 and img_counts[nth - 1, :, 0].sum() == N         # at the lowest threshold every image holds its true positive
    terms = np.array([(1.0 + np.cos(g["alpha"][0] - d["alpha"][0])) / 2.0 for g, d in zip(gt, dt)])
    tp = img_counts[:nth, :, 0] == 1
    worst = np.abs(img_sim[:nth] - terms[None])[tp].max()
    print(f"aos: worst |device term - numpy term| over {int(tp.sum())} single-true-positive cells = {worst:.3e} = {worst / ULP1:.2f} ulp of 1.0")
    assert worst <= TERM <= 4 * ULP1
    score = np.array([d["score"][0] for d in dt])
    for ti in range(nth):
        host = 0.0
        n = 0
        for i in range(N):                                            # eval_class: pr[t, 3] += sim, image by image
            if score[i] >= thr[ti]:
                host += terms[i]
                n += 1
        assert n == img_counts[ti, :, 0].sum() > 0
        bound = 2 * (n - 1) * 2.0 ** -53 * host + n * TERM
        assert abs(pr_sim[ti] - host) <= bound, (ti, pr_sim[ti] - host, bound)
    ref = ke.eval_class(gt, dt, [0], [0], 0, mo, compute_aos=True)
    dev = ke.eval_class_device(p, [0], [0], 0, mo, compute_aos=True)
    assert np.array_equal(dev["precision"], ref["precision"], equal_nan=True)
    assert np.abs(dev["orientation"] - ref["orientation"]).max() <= 2 * (N - 1) * 2.0 ** -53 + TERM      # sums over <= N terms divided by tp + fp >= their count


# ----------------------------------------------------------------------------- 8: rows from the device
def test_with_rows_equals_packing_the_formatted_rows():
    from minddet.models import Config, build_detector
    from minddet_amd import det_ops
    from minddet_amd import kitti_eval as ke
    from tests.kitti_io_cases import CAR_RANGE, calibration, detections
    cal = calibration((0, 1), device=DEV)
    dets = detections(9, 2, 40, cal)
    names = ["Car", "Pedestrian", "Cyclist"]
    count = torch.tensor([0, 37], dtype=torch.int32, device=DEV)
    rows, src, out_count = det_ops.kitti_rows(torch.from_numpy(dets).to(DEV), count, cal.tensor("lidar2cam"), cal.tensor("p2"), cal.tensor("image_shape"),
                                              limit_range=CAR_RANGE)
    annos = ke.rows_to_annos(rows, src, out_count, None, names, [7, 8])
    n = len(annos[1]["name"])
    assert len(annos[0]["name"]) == 0 and 20 < n <= 37
    rng = np.random.default_rng(4)
    gt = []
    for a in annos:                                                   # ground truth: the detections jittered, of every difficulty, and a DontCare box
        k = len(a["name"])
        g = dict(name=np.concatenate([a["name"], ["DontCare"]]), bbox=np.concatenate([a["bbox"].reshape(-1, 4) + rng.normal(0, 1.0, (k, 4)), [[0.0, 0.0, 50.0, 50.0]]]),
                 location=np.concatenate([a["location"].reshape(-1, 3) + rng.normal(0, 0.1, (k, 3)), [[-1000.0] * 3]]),
                 dimensions=np.concatenate([a["dimensions"].reshape(-1, 3), [[-1.0] * 3]]), rotation_y=np.concatenate([a["rotation_y"] + rng.normal(0, 0.05, k), [-10.0]]),
                 alpha=np.concatenate([a["alpha"] + rng.normal(0, 0.1, k), [-10.0]]), occluded=np.concatenate([rng.integers(0, 3, k), [-1]]),
                 truncated=np.concatenate([rng.choice([0.0, 0.2, 0.4], k), [-1.0]]))
        gt.append(g)
    want = ke.pack_annos(gt, annos, device=DEV)
    got = ke.pack_annos(gt, None, device=DEV).with_rows(rows, out_count, names)
    total = int(want.dt_off[-1])
    assert total == n and torch.equal(got.dt_off, want.dt_off) and torch.equal(got.ov_off, want.ov_off) and got.pairs >= want.pairs
    for key in ke.PackedEval.DT:
        g, w = getattr(got, key), getattr(want, key)
        g = g[:, :total] if key == "dt_same" else g[:total]
        assert g.dtype == w.dtype and g.shape == w.shape and g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes(), key
        rest = getattr(got, key)
        assert not (rest[:, total:] if key == "dt_same" else rest[total:]).any()                       # the capacity behind the detections is zero
    assert got.dt_box.shape == (2 * 40, 4) and got.compute_aos and want.compute_aos
    tiny = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", "pointpillars_tiny_kitti.py"))
    det = build_detector(dict(tiny.model), None, tiny.test_cfg)
    text, out = det.evaluate_kitti(rows, out_count, gt, names)
    ref_text, ref_out = ke.get_official_eval_result(gt, annos, [0, 1, 2])
    assert set(out) == set(ref_out) and "Car_aos/easy_R40" in out and max(out.values()) > 1
    for k in out:                                                     # AOS: percent of a mean of sums within the bound of test 7, far below 1e-10
        assert out[k] == ref_out[k] or ("aos" in k and abs(out[k] - ref_out[k]) <= 1e-10), (k, out[k], ref_out[k])
    assert [l for l in text.splitlines() if not l.startswith("aos")] == [l for l in ref_text.splitlines() if not l.startswith("aos")]
