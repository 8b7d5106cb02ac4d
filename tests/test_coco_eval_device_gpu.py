"""-m gpu: the COCO bbox AP evaluation on the device (include/minddet_hip_cocoeval.h) judged by the host evaluator it replaces
(minddet_amd/coco_eval.py: dets_to_coco, COCOBboxEval._evaluate_img, evaluate, summarize) -- never by itself.  Every comparison is
exact (np.array_equal on the values, the float tables on their bits), so there are no tolerances.  The set is
tests/coco_eval_contract.py's: 16 generated images x 3 categories plus the hand-made cells."""
import functools

import numpy as np
import pytest
import torch

from tests import coco_eval_contract as cc
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]

DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def _host():
    """the host evaluator on the test set, evaluated once and left unchanged"""
    from minddet_amd import coco_eval as ce
    gts, dts, imgs, cats, where = cc.test_set()
    return ce.COCOBboxEval(gts, dts, imgs, cats).evaluate(), where


@functools.lru_cache(maxsize=None)
def _device_tables():
    """pack_coco on the device and the two operators on it -> (pack as numpy, dtm, dt_ig, cell_ngt, precision, recall, n_gt)"""
    from minddet_amd import coco_eval as ce
    from minddet_amd import det_ops
    EV = ce.COCOBboxEval
    gts, dts, imgs, cats, _ = cc.test_set()
    p = ce.pack_coco(gts, dts, imgs, cats, device=DEV)
    const = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(DEV)
    dtm, dt_ig, cell_ngt = det_ops.coco_eval_match(p.gt_beg, p.gt_cnt, p.dt_beg, p.dt_cnt, p.gt_box, p.gt_area, p.gt_crowd, p.gt_ignore, p.dt_box, p.dt_area,
                                                   const(EV.IOU_THRS, np.float64), const(list(EV.AREA_RNG.values()), np.float64))
    order, cat_off = p.category_order()
    out = det_ops.coco_eval_accumulate(order, cat_off, p.dt_rank, dtm, dt_ig, cell_ngt, const(EV.REC_THRS, np.float64), const(EV.MAX_DETS, np.int32))
    return (cc.pack_numpy(p),) + tuple(t.cpu().numpy() for t in (dtm, dt_ig, cell_ngt) + out)


def test_match_tables_equal_evaluate_img_for_every_cell_area_range_and_threshold():
    from minddet_amd import coco_eval as ce
    ev, where = _host()
    z, dtm, dt_ig, cell_ngt = _device_tables()[:4]
    Kc, seen = len(ev.cat_ids), dict(matched=0, ignored=0, crowd_twice=0)
    inside = np.zeros(len(z["dt_area"]), bool)
    for i, img in enumerate(ev.img_ids):
        for k, cat in enumerate(ev.cat_ids):
            c = i * Kc + k
            ds = slice(z["dt_beg"][c], z["dt_beg"][c] + z["dt_cnt"][c])
            inside[ds] = True
            for a, rng in enumerate(ce.COCOBboxEval.AREA_RNG.values()):
                e = ev._evaluate_img(img, cat, rng, 100)
                if e is None:
                    assert z["gt_cnt"][c] == 0 and z["dt_cnt"][c] == 0 and cell_ngt[a, c] == 0
                    continue
                gts = ev.gts.get((img, cat), [])
                g_ig = np.array([g["_ignore"] or g["area"] < rng[0] or g["area"] > rng[1] for g in gts], bool)
                back = np.append(np.argsort(g_ig, kind="mergesort") + z["gt_beg"][c], -1)     # the host's index through its ground-truth order
                assert np.array_equal(dtm[a][:, ds], back[e["dtm"]]), (img, cat, a)
                assert np.array_equal(dt_ig[a][:, ds] != 0, e["dt_ig"]), (img, cat, a)
                assert cell_ngt[a, c] == e["n_gt"], (img, cat, a)
                seen["matched"] += int((e["dtm"] >= 0).sum())
                seen["ignored"] += int(e["dt_ig"].sum())
                for t in range(e["dtm"].shape[0]):
                    hit = e["dtm"][t][e["dtm"][t] >= 0]
                    seen["crowd_twice"] += len(hit) - len(set(hit.tolist()))
    assert inside.all() and min(seen.values()) > 0, seen
    # the hand-made cells say what they were made for
    cell = lambda name: ev.img_ids.index(where[name][0]) * Kc + ev.cat_ids.index(where[name][1])
    rows = lambda name: slice(z["dt_beg"][cell(name)], z["dt_beg"][cell(name)] + z["dt_cnt"][cell(name)])
    assert (dtm[0][:, rows("dets_only")] == -1).all() and cell_ngt[0, cell("gts_only")] == 2 and z["dt_cnt"][cell("gts_only")] == 0
    assert z["dt_cnt"][cell("dets_140")] == 100 and (dtm[0][0, rows("dets_140")] >= 0).sum() == 2
    assert cell_ngt[0, cell("all_crowd")] == 0 and (dt_ig[0][0, rows("all_crowd")] != 0).sum() == 3
    half = dtm[0][:, rows("iou_half")]                               # IoU exactly 0.5 and 0.75 meet their thresholds, and no higher one
    assert (half[:, 0] >= 0).tolist() == [True] + [False] * 9 and (half[:, 1] >= 0).tolist() == [True] * 6 + [False] * 4
    three_fifths = dtm[0][:, rows("iou_three_fifths")][:, 0] >= 0
    assert three_fifths.tolist() == [bool(0.6 >= t) for t in ce.COCOBboxEval.IOU_THRS]
    g0 = z["gt_beg"][cell("crowd_and_counted")]
    assert dtm[0][0, rows("crowd_and_counted")].tolist() == [g0] and dtm[0][8, rows("crowd_and_counted")].tolist() == [g0 + 1]
    for n in (65, 130, 256):
        got = dtm[0][0, rows(f"gts_{n}")] - z["gt_beg"][cell(f"gts_{n}")]
        assert got.max() == n - 1 and len({g // 64 for g in got.tolist() if g >= 0}) == (n + 63) // 64      # a match in every chunk


def test_precision_and_recall_equal_the_host_tables():
    ev, _ = _host()
    precision, recall, n_gt = _device_tables()[4:]
    assert precision.shape == ev.precision.shape and recall.shape == ev.recall.shape
    assert np.array_equal(_bits(precision), _bits(ev.precision)) and np.array_equal(_bits(recall), _bits(ev.recall))
    k4, k5 = ev.cat_ids.index(4), ev.cat_ids.index(5)
    assert (precision[:, :, k4] == -1).all() and (recall[:, k4] == -1).all() and (n_gt[:, k4] == 0).all()       # no ground truth
    assert (precision[:, :, k5, 0] == 0).all() and (recall[:, k5, 0] == 0).all() and n_gt[0, k5] == 2             # ground truths, no detection
    k3 = ev.cat_ids.index(3)                                         # the lattice cells: more than 10 detections per cell, so all three maxDets differ
    assert 0 < recall[0, k3, 0, 0] < recall[0, k3, 0, 1] < recall[0, k3, 0, 2]
    assert ((precision > 0) & (precision < 1)).any()


def _f32_dets(seed=5, B=5, max_det=160):
    rng = np.random.default_rng(seed)
    dets = np.zeros((B, max_det, 6), np.float32)
    dets[..., :2] = rng.integers(0, 800, (B, max_det, 2)) / 8                     # k/8 coordinates: .125 ties of to_float
    dets[..., 2:4] = dets[..., :2] + rng.integers(1, 900, (B, max_det, 2)) / 8
    dets[..., 4] = rng.choice([0.125, 0.375, 0.625, 0.3, 0.9, 0.905, 0.0], (B, max_det))
    dets[..., 5] = rng.integers(0, 4, (B, max_det))
    dets[1, :130, 5] = 3                                                         # more than 100 rows of one class in one image
    dets[3, ::7, :4] += np.float32(0.3)                                          # and coordinates off the grid
    return dets, np.array([max_det, max_det - 10, 0, 77, 1], np.int32)


def test_rows_equal_dets_to_coco_and_pack_coco():
    from minddet_amd import coco_eval as ce
    dets, count = _f32_dets()
    imgs, valid_ids, cat_ids = [3, 5, 6, 7, 9, 11], [10, 20, 77, 40], [10, 20, 40]      # label 2 has no category: dropped; image 11 gets no batch
    ref = ce.dets_to_coco(dets, count, imgs[:5], valid_ids)
    z = cc.pack_numpy(ce.pack_coco([], [r for r in ref if r["category_id"] in cat_ids], imgs, cat_ids, device="cpu"))
    p = ce.pack_coco([], None, imgs, cat_ids, device=DEV)
    td, tc = torch.from_numpy(dets).to(DEV), torch.from_numpy(count).to(DEV)
    p.add_dets(td[3:5], tc[3:5], 3, valid_ids)                                    # two batches, the later images first
    p.add_dets(td[:3], tc[:3], 0, valid_ids)
    got = {n: getattr(p, n).cpu().numpy() for n in ("dt_box", "dt_area", "dt_score", "dt_cat", "dt_rank", "dt_beg", "dt_cnt", "dt_src")}
    M, Kc = dets.shape[1], 3
    assert np.array_equal(got["dt_cnt"], z["dt_cnt"]) and z["dt_cnt"].max() == 100 and got["dt_cnt"][5 * Kc:].sum() == 0
    used = np.zeros(len(got["dt_cat"]), bool)
    for i in range(len(imgs)):
        assert got["dt_beg"][i * Kc] == i * M
        for k in range(Kc):
            c, n = i * Kc + k, int(z["dt_cnt"][i * Kc + k])
            a, b = int(got["dt_beg"][c]), int(z["dt_beg"][c])
            assert k == 0 or a == got["dt_beg"][c - 1] + got["dt_cnt"][c - 1]
            for name in ("dt_box", "dt_area", "dt_score"):
                assert np.array_equal(_bits(got[name][a:a + n]), _bits(z[name][b:b + n])), (i, k, name)
            assert np.array_equal(got["dt_cat"][a:a + n], z["dt_cat"][b:b + n]) and np.array_equal(got["dt_rank"][a:a + n], z["dt_rank"][b:b + n])
            if i < 5:                                                             # the source rows: the class's rows in order, by the rounded score, stable
                src = [r for r in range(count[i]) if valid_ids[int(dets[i, r, 5])] == cat_ids[k]]
                by = np.argsort([-ce.to_float(float(dets[i, r, 4])) for r in src], kind="mergesort")[:100]
                assert got["dt_src"][a:a + n].tolist() == [src[j] for j in by], (i, k)
            used[a:a + n] = True
    assert (got["dt_cat"][~used] == Kc).all() and (got["dt_src"][~used] == -1).all() and (got["dt_score"][~used] == 0).all()
    assert np.signbit(got["dt_box"]).sum() == 0 and (z["dt_score"] == 0.12).any() and (z["dt_score"] == 0.38).any() and (z["dt_score"] == 0.9).any()


def test_summaries_equal_the_hosts_from_records_and_from_device_detections():
    from minddet_amd import coco_eval as ce
    ev, _ = _host()
    gts, dts, imgs, cats, _ = cc.test_set()
    got = ce.COCOBboxEval(gts, dts, imgs, cats).evaluate(backend="device", device=DEV).summarize()
    assert got == ev.summarize() and got["AP"] > 0.1
    # detections that exist only on the device: the detector's (dets, count), two batches
    rng = np.random.default_rng(9)
    B, M = len(imgs), 48
    dets, count = np.zeros((B, M, 6), np.float32), np.zeros(B, np.int32)
    by_img = {}
    for g in gts:
        by_img.setdefault(g["image_id"], []).append(g)
    for b, img in enumerate(imgs):
        some = by_img.get(img, [])[:40]
        for r, g in enumerate(some):                                              # around the ground truths, on a k/8 grid, tied scores
            x, y, w, h = g["bbox"]
            dx, dy = rng.integers(-16, 17, 2) / 8
            dets[b, r] = [x + dx, y + dy, x + dx + w, y + dy + h, rng.choice([0.125, 0.5, 0.625, 0.9]), cats.index(g["category_id"])]
        count[b] = len(some)
    host = ce.COCOBboxEval(gts, ce.dets_to_coco(dets, count, imgs, cats), imgs, cats).evaluate()
    p = ce.pack_coco(gts, None, imgs, cats, device=DEV)
    td, tc = torch.from_numpy(dets).to(DEV), torch.from_numpy(count).to(DEV)
    p.add_dets(td[:10], tc[:10], 0).add_dets(td[10:], tc[10:], 10)
    dev = ce.COCOBboxEval.from_packed(p).evaluate(backend="device")
    assert np.array_equal(_bits(dev.precision), _bits(host.precision)) and np.array_equal(_bits(dev.recall), _bits(host.recall))
    assert dev.summarize() == host.summarize() and host.summarize()["AP"] > 0.1


@pytest.mark.parametrize("empty", ["detections", "ground truth", "both"])
def test_empty_sets_give_the_hosts_tables(empty):
    from minddet_amd import coco_eval as ce
    gts, dts, imgs, cats, _ = cc.test_set()
    gts, dts = gts[:60], dts[:80]
    gts, dts = ([] if empty != "detections" else gts), ([] if empty != "ground truth" else dts)
    host = ce.COCOBboxEval(gts, dts, imgs, cats).evaluate()
    dev = ce.COCOBboxEval(gts, dts, imgs, cats).evaluate(backend="device", device=DEV)
    assert np.array_equal(_bits(dev.precision), _bits(host.precision)) and np.array_equal(_bits(dev.recall), _bits(host.recall))
    assert dev.summarize() == host.summarize()
    assert (host.precision == -1).all() if empty != "detections" else (host.precision == 0).any()


def test_two_calls_give_identical_bytes():
    from minddet_amd import coco_eval as ce
    from minddet_amd import det_ops
    z, dtm, dt_ig, cell_ngt, precision, recall, n_gt = _device_tables()
    _device_tables.cache_clear()
    again = _device_tables()
    for a, b in zip((dtm, dt_ig, cell_ngt, precision, recall, n_gt), again[1:]):
        assert a.tobytes() == b.tobytes()
    dets, count = _f32_dets()
    td, tc = torch.from_numpy(dets).to(DEV), torch.from_numpy(count).to(DEV)
    outs = []
    for fill in (0, 0x5a):                                            # the operands start from different bytes: every element of the batch's images is written
        I, M, Kc = 5, dets.shape[1], 3
        ops = [torch.empty(s, dtype=dt, device=DEV) for s, dt in (((I * M, 4), torch.float64), ((I * M,), torch.float64), ((I * M,), torch.float64), ((I * M,), torch.int32),
                                                                  ((I * M,), torch.int32), ((I * Kc,), torch.int32), ((I * Kc,), torch.int32), ((I * M,), torch.int32))]
        for t in ops:
            t.view(torch.uint8).fill_(fill)
        det_ops.coco_eval_rows(td, tc, torch.tensor([0, 1, -1, 2], dtype=torch.int32, device=DEV), 0, *ops)
        outs.append([t.cpu().numpy().tobytes() for t in ops])
    assert outs[0] == outs[1]
