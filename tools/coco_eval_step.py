"""Times the COCO bbox AP evaluation on the device (csrc/cocoeval.hip) on a synthetic set of the shape of COCO val2017 -- 5 000 images, 80
categories, about 7 ground truths and 100 detections per image, the detections drawn around ground truths so AP is not near zero -- and
prints ONE JSON line (also written to --out).

  images, categories, gt_rows, dt_rows   the packed extents (dt_rows = images x max_det, the padded layout of md_coco_eval_rows)
  pack_ms        coco_eval.pack_coco of the ground truth: host grouping and the upload, wall time, per round
  rows_ms        PackedCoco.add_dets over all images in batches of --batch (md_coco_eval_rows), the detections already on the device
  match_ms       md_coco_eval_match; sorts_ms: PackedCoco.category_order (two stable torch sorts and a count); accumulate_ms:
                 md_coco_eval_accumulate.  Event-timed, `steps` calls each, in three interleaved rounds (round r times every stage before
                 round r + 1 starts); the figure is the median of the rounds
  device_total_ms  from_packed(...).evaluate(backend="device") + summarize() on the packed set, wall time, the read of the tables included
  host_subset_ms   dets_to_coco + COCOBboxEval.evaluate() + summarize() on the FIRST --host-images images only, wall time: the host on
                   all images takes minutes.  host_scaled_ms = host_subset_ms / host_images x images is an extrapolation, not a measurement
  device_subset_ms the device path on the same subset; subset_equal: the two summaries are the same dict, the tables the same bits
Not measured: real detections (these are jittered ground truth and strays), the host evaluator on the whole set.

python tools/coco_eval_step.py [--images 5000] [--host-images 100] [--steps 5] [--out profiles/coco_eval_device.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from minddet_amd import coco_eval as ce  # noqa: E402
from minddet_amd import det_ops  # noqa: E402

DEV = "cuda:0"


def synthetic(rng, n_img, n_cat, max_det):
    """-> (ground-truth records, dets [I, max_det, 6] f32, count [I] i32): per image a Poisson(7) number of boxes, 8 % crowds; every box
    found with probability 0.8 (jittered, sometimes with the wrong label), the rest of the max_det rows strays with low scores"""
    gts = []
    dets, count = np.zeros((n_img, max_det, 6), np.float32), np.full(n_img, max_det, np.int32)
    for i in range(n_img):
        n = int(rng.poisson(7))
        wh = rng.uniform(12, 260, (n, 2))
        xy = rng.uniform(0, 640 - 12, (n, 2))
        cat = rng.integers(0, n_cat, n)
        for j in range(n):
            gts.append(dict(image_id=i + 1, category_id=int(cat[j]) + 1, bbox=[round(float(v), 2) for v in (*xy[j], *wh[j])], iscrowd=int(rng.random() < 0.08)))
        found = np.flatnonzero(rng.random(n) < 0.8)[:max_det]
        k = len(found)
        box = np.concatenate([xy[found] + rng.normal(0, 0.06, (k, 2)) * wh[found], wh[found] * rng.normal(1, 0.08, (k, 2))], 1)
        stray = np.concatenate([rng.uniform(0, 600, (max_det - k, 2)), rng.uniform(10, 200, (max_det - k, 2))], 1)
        box = np.concatenate([box, stray])
        dets[i, :, :2], dets[i, :, 2:4] = box[:, :2], box[:, :2] + box[:, 2:]
        dets[i, :, 4] = np.concatenate([rng.uniform(0.3, 1.0, k), rng.uniform(0.01, 0.5, max_det - k)])
        dets[i, :, 5] = np.concatenate([np.where(rng.random(k) < 0.9, cat[found], rng.integers(0, n_cat, k)), rng.integers(0, n_cat, max_det - k)])
    return gts, dets, count


def time_calls(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--categories", type=int, default=80)
    ap.add_argument("--max-det", type=int, default=100)
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--host-images", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_eval_device.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("coco_eval_step: needs the GPU (a time taken anywhere else says nothing)")
    EV = ce.COCOBboxEval
    gts, dets, count = synthetic(np.random.default_rng(args.seed), args.images, args.categories, args.max_det)
    imgs, cats = list(range(1, args.images + 1)), list(range(1, args.categories + 1))
    td, tc = torch.from_numpy(dets).to(DEV), torch.from_numpy(count).to(DEV)
    const = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(DEV)
    iou_thr, rec_thr = const(EV.IOU_THRS, np.float64), const(EV.REC_THRS, np.float64)
    area_rng, max_dets = const(list(EV.AREA_RNG.values()), np.float64), const(EV.MAX_DETS, np.int32)

    def add_all(p, n=args.images):
        for b in range(0, n, args.batch):
            p.add_dets(td[b:min(b + args.batch, n)], tc[b:min(b + args.batch, n)], b)
        return p

    p = add_all(ce.pack_coco(gts, None, imgs, cats, device=DEV))
    match = lambda: det_ops.coco_eval_match(p.gt_beg, p.gt_cnt, p.dt_beg, p.dt_cnt, p.gt_box, p.gt_area, p.gt_crowd, p.gt_ignore, p.dt_box, p.dt_area, iou_thr, area_rng)
    dtm, dt_ig, cell_ngt = match()
    order, cat_off = p.category_order()
    accumulate = lambda: det_ops.coco_eval_accumulate(order, cat_off, p.dt_rank, dtm, dt_ig, cell_ngt, rec_thr, max_dets)
    accumulate()
    torch.cuda.synchronize()
    rounds = {k: [] for k in ("pack", "rows", "match", "sorts", "accumulate")}
    for _ in range(3):                                                # interleaved: every stage once per round
        rounds["pack"].append(wall(lambda: ce.pack_coco(gts, None, imgs, cats, device=DEV))[0])
        rounds["rows"].append(time_calls(lambda: add_all(p), args.steps))
        rounds["match"].append(time_calls(match, args.steps))
        rounds["sorts"].append(time_calls(p.category_order, args.steps))
        rounds["accumulate"].append(time_calls(accumulate, args.steps))
    res = dict(metric="coco_eval_device", images=args.images, categories=args.categories, max_det=args.max_det, batch=args.batch, steps=args.steps,
               gt_rows=int(p.gt_box.shape[0]), dt_rows=int(p.dt_box.shape[0]), dt_used=int(cat_off[-1]))
    for key, v in rounds.items():
        res[key + "_ms"] = round(statistics.median(v), 4)
        res[key + "_rounds_ms"] = [round(t, 4) for t in v]
    res["device_ops_sum_ms"] = round(sum(statistics.median(rounds[k]) for k in ("rows", "match", "sorts", "accumulate")), 3)
    total_ms, summary = wall(lambda: EV.from_packed(p).evaluate(backend="device").summarize())
    res.update(device_total_ms=round(total_ms, 2), AP=round(summary["AP"], 4), AP50=round(summary["AP50"], 4), AR100=round(summary["AR100"], 4))
    n = min(args.host_images, args.images)
    sub_gts = [g for g in gts if g["image_id"] <= n]
    host_ms, host = wall(lambda: EV(sub_gts, ce.dets_to_coco(dets[:n], count[:n], imgs[:n], cats), imgs[:n], cats).evaluate())
    dev_ms, dev = wall(lambda: EV.from_packed(add_all(ce.pack_coco(sub_gts, None, imgs[:n], cats, device=DEV), n)).evaluate(backend="device"))
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    res.update(host_images=n, host_subset_ms=round(host_ms, 1), device_subset_ms=round(dev_ms, 2), host_ms_per_image=round(host_ms / n, 2),
               host_scaled_ms=round(host_ms / n * args.images, 0), host_scaled_is_extrapolated=True,
               subset_equal=bool(host.summarize() == dev.summarize() and np.array_equal(bits(host.precision), bits(dev.precision))
                                 and np.array_equal(bits(host.recall), bits(dev.recall))))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
