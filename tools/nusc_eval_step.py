"""Times the nuScenes detection evaluation on the device (csrc/nusceval.hip) on a synthetic set of the shape of the nuScenes val split -- 6 019
samples, 10 classes, 498 rows per sample (six tasks x 83), about 35 ground truths per sample -- and writes one JSON line
(profiles/nusc_eval_device.json):

  samples, classes, gt_rows, dt_rows, dt_used   the packed extents (dt_rows = samples x max_det, the padded layout of md_nusc_rows)
  pack_ms        nusc_eval.pack_nusc of the ground truth: host filter, grouping and the upload, wall time, per round
  rows_ms        PackedNusc.add_dets over all samples in batches of --batch (md_nusc_rows), the detections already on the device
  match_ms       md_nusc_eval_match; sorts_ms: PackedNusc.category_order (three stable torch sorts and a count); accumulate_ms:
                 md_nusc_eval_accumulate.  Event-timed, `steps` calls each, in three interleaved rounds (round r times every stage before
                 round r + 1 starts); the medians and the rounds
  device_total_ms   NuscDetectionEval.from_packed(p).evaluate(backend="device").summarize(), wall time with the read of the five tables
  host_*         the host judge on the first --host-samples samples: dets_to_nusc (host_format_ms) and NuscDetectionEval(...).evaluate()
                 on rows_to_results of the device rows (host_subset_ms); the device on the same subset; subset_equal: the tables and the
                 summary agree bit for bit.  host_scaled_ms is host_subset_ms scaled to all samples: an extrapolation, not a measurement
The serial running-sum part of the accumulate kernel is not timed separately here (no kernel trace is taken).

python tools/nusc_eval_step.py [--samples 6019] [--host-samples 100] [--steps 5] [--out profiles/nusc_eval_device.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from minddet_amd import det_ops  # noqa: E402
from minddet_amd import nusc_eval as ne  # noqa: E402

DEV = "cuda:0"
CLASSES = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone")


def synthetic(rng, n_smp, max_det):
    """-> (ground-truth records, dets [I, max_det, 11] f32, count [I] i32, poses [I, 14]): per sample a Poisson(35) number of boxes within
    45 m of the sensor; every box found with probability 0.8 (jittered by 0.3 m, sometimes with the wrong label), the rest of the rows
    strays with low scores"""
    gts = []
    dets, count, poses = np.zeros((n_smp, max_det, 11), np.float32), np.full(n_smp, max_det, np.int32), np.zeros((n_smp, 14))
    for i in range(n_smp):
        a = rng.uniform(-math.pi, math.pi)
        poses[i] = [1, 0, 0, 0, 0.94, 0.0, 1.84, math.cos(a / 2), 0, 0, math.sin(a / 2), rng.uniform(300, 2000), rng.uniform(300, 2000), 0.0]
        n = int(rng.poisson(35))
        box = np.zeros((max_det, 11), np.float32)
        k = min(int((rng.random(n) < 0.8).sum()), max_det)
        box[:, :2] = rng.uniform(-45, 45, (max_det, 2))
        box[:, 2] = rng.uniform(-2, 0, max_det)
        box[:, 3:6] = rng.uniform(0.4, 6, (max_det, 3))
        box[:, 6:8] = rng.normal(0, 2, (max_det, 2)) * (rng.random((max_det, 1)) < 0.4)
        box[:, 8] = rng.uniform(-math.pi, math.pi, max_det)
        box[:, 9] = np.concatenate([rng.uniform(0.3, 1.0, k), rng.uniform(0.1, 0.4, max_det - k)])
        box[:, 10] = rng.integers(0, 10, max_det)
        dets[i] = box
        truth = box[:n].copy() if n <= max_det else box.copy()
        truth[:, :2] += rng.normal(0, 0.3, (len(truth), 2)).astype(np.float32)
        truth[:k, 10] = np.where(rng.random(k) < 0.9, truth[:k, 10], rng.integers(0, 10, k))
        for t in truth:
            c, size, q, v = ne.box_to_global(t[:9], poses[i])
            name = CLASSES[int(t[10])]
            gts.append({"sample_token": i, "translation": c.tolist(), "size": size.tolist(), "rotation": q.tolist(), "velocity": v[:2].tolist(),
                        "detection_name": name, "attribute_name": "" if name in ("barrier", "traffic_cone") else ne.DEFAULT_ATTR[name], "num_pts": 5})
    return gts, dets, count, poses


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
    ap.add_argument("--samples", type=int, default=6019)
    ap.add_argument("--max-det", type=int, default=498)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--host-samples", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nusc_eval_device.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nusc_eval_step: needs the GPU (a time taken anywhere else says nothing)")
    gts, dets, count, poses = synthetic(np.random.default_rng(args.seed), args.samples, args.max_det)
    ego = poses[:, 11:14]
    td, tc, tp = torch.from_numpy(dets).to(DEV), torch.from_numpy(count).to(DEV), torch.from_numpy(poses).to(DEV)
    const = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV)

    def add_all(p, n=args.samples):
        for b in range(0, n, args.batch):
            e = min(b + args.batch, n)
            p.add_dets(td[b:e], tc[b:e], tp[b:e], b)
        return p

    p = add_all(ne.pack_nusc(gts, ego, CLASSES, device=DEV))
    ev = ne.NuscDetectionEval.from_packed(p)
    dist_thr, period, rec_thr, tpi = const(ev.cfg["dist_ths"]), const(ev.periods()), const(np.linspace(0, 1, 101)), ev.tp_index()
    match = lambda: det_ops.nusc_eval_match(p.gt_beg, p.gt_cnt, p.dt_beg, p.dt_cnt, p.gt_xy, p.gt_size, p.gt_yaw, p.gt_vel, p.gt_attr, p.dt_xyz, p.dt_size,
                                            p.dt_yaw, p.dt_vel, p.dt_attr, dist_thr, period, tpi)
    dtm, err, cell_ngt = match()
    order, cat_off = p.category_order()
    accumulate = lambda: det_ops.nusc_eval_accumulate(order, cat_off, p.dt_score, dtm, err, cell_ngt, rec_thr, tpi)
    accumulate()
    torch.cuda.synchronize()
    rounds = {k: [] for k in ("pack", "rows", "match", "sorts", "accumulate")}
    for _ in range(3):                                                # interleaved: every stage once per round
        rounds["pack"].append(wall(lambda: ne.pack_nusc(gts, ego, CLASSES, device=DEV))[0])
        rounds["rows"].append(time_calls(lambda: add_all(p), args.steps))
        rounds["match"].append(time_calls(match, args.steps))
        rounds["sorts"].append(time_calls(p.category_order, args.steps))
        rounds["accumulate"].append(time_calls(accumulate, args.steps))
    res = dict(metric="nusc_eval_device", samples=args.samples, classes=len(CLASSES), max_det=args.max_det, batch=args.batch, steps=args.steps,
               gt_rows=int(p.gt_xy.shape[0]), dt_rows=int(p.dt_xyz.shape[0]), dt_used=int(cat_off[-1]))
    for key, v in rounds.items():
        res[key + "_ms"] = round(statistics.median(v), 4)
        res[key + "_rounds_ms"] = [round(t, 4) for t in v]
    res["device_ops_sum_ms"] = round(sum(statistics.median(rounds[k]) for k in ("rows", "match", "sorts", "accumulate")), 3)
    total_ms, summary = wall(lambda: ne.NuscDetectionEval.from_packed(p).evaluate(backend="device").summarize())
    res.update(device_total_ms=round(total_ms, 2), mean_ap=round(summary["mean_ap"], 4), nd_score=round(summary["nd_score"], 4), serial_chain_ms=None)
    n = min(args.host_samples, args.samples)
    sub_gts = [g for g in gts if g["sample_token"] < n]
    fmt_ms, _ = wall(lambda: ne.dets_to_nusc(dets[:n], count[:n], poses[:n], CLASSES))
    sub = add_all(ne.pack_nusc(sub_gts, ego[:n], CLASSES, device=DEV), n)
    dev_ms, dev = wall(lambda: ne.NuscDetectionEval.from_packed(sub).evaluate(backend="device"))
    flat = [r for recs in ne.rows_to_results(sub)["results"].values() for r in recs]
    host_ms, host = wall(lambda: ne.NuscDetectionEval(sub_gts, flat, ego[:n], CLASSES).evaluate())
    same = lambda a, b: np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
    res.update(host_samples=n, host_format_ms=round(fmt_ms, 1), host_subset_ms=round(host_ms, 1), device_subset_ms=round(dev_ms, 2),
               host_ms_per_sample=round(host_ms / n, 2), host_scaled_ms=round(host_ms / n * args.samples, 0), host_scaled_is_extrapolated=True,
               subset_equal=bool(repr(host.summarize()) == repr(dev.summarize())
                                 and all(same(host.tables[k], dev.tables[k]) for k in ("precision", "confidence", "tp_err", "n_gt", "n_match"))))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
