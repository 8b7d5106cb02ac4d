"""Times the KITTI camera-frame ends (csrc/kitti.hip) at the shape of configs/pointpillars/pointpillars_car_xyres16_kitti.py -- B = 4 raw
velodyne scans of 120 000 points, a full turn of the scanner, KITTI-shaped calibrations -- and prints ONE JSON line (also written to --out).

  crop_ms / crop_torch_ms / crop_host_ms, rows_ms / rows_host_ms, forward_kitti_ms / forward_ms (+ *_rounds_ms)
                      median / each of three rounds of `steps` calls in one process, the rounds interleaved.  The device entries are
                      event-timed; the host entries are wall time around a call that ends with its result on the device (crop) or on
                      the host (rows), the copies included
  crop                det_ops.crop_hulls on the image frustum (md_pc_crop_hulls: four launches)
  crop_torch          the same result with torch device operators: the planes from the corners, pts.double() @ n.T + d for the six
                      signs, all(< 0), a cumsum of the kept flags and an index_copy_ into the zeroed output; the per-sample offsets
                      gathered from the cumsum: no host read, as the operator.  One hull per sample (the image frustum), the samples'
                      bounds host integers
  crop_host           the points copied to the host, tests/kitti_io_contract.py's crop in numpy float64, the result copied back
  rows                det_ops.kitti_rows on the detections forward() returned (random weights: the count is what it is)
  rows_host           the detections copied to the host, kitti_eval.lidar_boxes_to_prediction + predictions_to_kitti_annos per sample
  forward_kitti       the whole chain on the raw scan; forward: the model alone on the cropped cloud
  floor_bytes / floor_us / floor_share
                      the crop's algorithmic traffic -- every input row read once (16 bytes), every output row written once (16 bytes,
                      kept or zero), one keep byte per row -- / --tbps (default 6.0 TB/s), and that time as a fraction of crop_ms.
                      moved_bytes: what this implementation moves (the keep byte read again twice, the kept rows read again)
  equal_to_contract   the device crop and rows meet the contract on this input; crop_torch_equal: the torch composition gives the same
                      rows and offsets

python tools/pointpillars_kitti_io_step.py [--steps 20] [--out profiles/pointpillars_kitti_io_step_b4.json]
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
from minddet.models import Config, build_detector  # noqa: E402
from minddet_amd import det_ops, kitti_eval  # noqa: E402
from tests import kitti_io_contract as kc  # noqa: E402
from tests.kitti_io_cases import calibration, scan  # noqa: E402

DEV = "cuda:0"


def time_calls(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def wall_calls(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def torch_crop(points, bounds, hulls, table):
    """the operator's result for one hull per sample with torch device operators -> (points_out [N,4], offsets [B+1])"""
    N = points.shape[0]
    s = hulls[:, 0][:, table]                                   # [B,6,4,3]
    a, b = s[:, :, 0] - s[:, :, 1], s[:, :, 1] - s[:, :, 2]
    n = torch.cross(a, b, dim=-1)
    d = -(n * s[:, :, 0]).sum(-1)
    keep = []
    for i in range(len(bounds) - 1):
        p = points[bounds[i]:bounds[i + 1], :3].double()
        keep.append(((p @ n[i].T + d[i]) < 0).all(1))
    keep = torch.cat(keep)
    csum = torch.cumsum(keep, 0)
    out = torch.zeros((N + 1, 4), dtype=torch.float32, device=points.device)
    out.index_copy_(0, torch.where(keep, csum - 1, N), points)
    offsets = torch.cat([csum.new_zeros(1), csum])[torch.as_tensor(bounds, device=points.device)].int()
    return out[:N], offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tbps", type=float, default=6.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointpillars_kitti_io_step_b4.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointpillars_kitti_io_step: needs the GPU (a time taken anywhere else says nothing)")
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", "pointpillars_car_xyres16_kitti.py"))
    model = build_detector(dict(cfg.model), cfg.train_cfg, cfg.test_cfg).to(DEV)
    B, n = args.batch, args.points
    cal = calibration(tuple(i % 2 for i in range(B)), DEV)
    pts = np.concatenate([scan(args.seed + i, n) for i in range(B)])
    bounds = [i * n for i in range(B + 1)]
    N = len(pts)
    points, offsets = torch.from_numpy(pts).to(DEV), torch.tensor(bounds, dtype=torch.int32, device=DEV)
    hulls, ones = cal.image_frustum(), cal.tensor("image_count")
    table = torch.from_numpy(kc.SURFACES).to(DEV)
    crop_out = torch.empty((N, 4), dtype=torch.float32, device=DEV)
    limit = cfg.test_cfg["post_center_limit_range"]
    names = list(model.class_names)

    def crop():
        return det_ops.crop_hulls(points, offsets, hulls, ones, out=crop_out)

    cpts, coffs, _ = (t.clone() for t in crop())
    dets, count = model.forward(cpts, coffs)
    l2c, p2, shape = cal.tensor("lidar2cam"), cal.tensor("p2"), cal.tensor("image_shape")

    def crop_host():
        c = kc.crop_hulls(points.cpu().numpy(), bounds, cal.image_frustum_host(), [1] * B)
        return torch.from_numpy(c["points"]).to(DEV), torch.from_numpy(c["offsets"]).to(DEV)

    def rows():
        return det_ops.kitti_rows(dets, count, l2c, p2, shape, limit_range=limit, lidar_input=False)

    def rows_host():
        d, k = dets.cpu().numpy(), count.cpu().numpy()
        preds = [kitti_eval.lidar_boxes_to_prediction(d[b, :k[b], :7], d[b, :k[b], 8], d[b, :k[b], 7], cal.rect[b], cal.trv2c[b], cal.p2[b], b)
                 for b in range(B)]
        return kitti_eval.predictions_to_kitti_annos(preds, cal.image_shape, names, limit, False)

    device = dict(crop=crop, crop_torch=lambda: torch_crop(points, bounds, hulls, table), rows=rows,
                  forward_kitti=lambda: model.forward_kitti(points, offsets, cal), forward=lambda: model.forward(cpts, coffs))
    host = dict(crop_host=crop_host, rows_host=rows_host)
    for fn in list(device.values()) + list(host.values()):
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in list(device) + list(host)}
    for _ in range(3):
        for k, fn in device.items():
            rounds[k].append(time_calls(fn, args.steps))
        for k, fn in host.items():
            rounds[k].append(wall_calls(fn, max(1, args.steps // 10)))
    med = {k: statistics.median(v) for k, v in rounds.items()}

    got = [t.cpu().numpy() for t in crop()]
    want = kc.crop_hulls(pts, bounds, cal.image_frustum_host(), [1] * B)
    r = [t.cpu().numpy() for t in rows()]
    rc = kc.kitti_rows(dets.cpu().numpy(), count.cpu().numpy(), cal.lidar2cam, cal.p2, cal.image_shape, limit, False)
    try:
        kc.check_crop(got[0], got[1], got[2], want, "crop")
        kc.check_rows(r[0], r[1], r[2], rc, "rows")
        equal = True
    except AssertionError as e:
        print("contract:", e, file=sys.stderr)
        equal = False
    tp, toffs = (t.cpu().numpy() for t in torch_crop(points, bounds, hulls, table))
    kept = int(got[1][-1])
    floor = N * 16 + N * 16 + N
    moved = N * 16 + N + 2 * N + kept * 16 + N * 16 + B * (192 + 2 * 192)
    res = dict(metric="pointpillars_kitti_io_step", config="pointpillars_car_xyres16_kitti", batch=B, points_per_sample=n, rows_in=N, rows_out=kept,
               dets_in=int(count.sum()), rows_reported=int(r[2].sum()), steps=args.steps, tbps=args.tbps, crop_launches_per_call=4, rows_launches_per_call=1,
               launches_traced=False)
    for key in rounds:
        res[key + "_ms"] = round(med[key], 4)
        res[key + "_rounds_ms"] = [round(t, 4) for t in rounds[key]]
    res.update(crop_torch_over_crop=round(med["crop_torch"] / med["crop"], 2), crop_host_over_crop=round(med["crop_host"] / med["crop"], 1),
               rows_host_over_rows=round(med["rows_host"] / med["rows"], 1), floor_bytes=floor, floor_us=round(floor / args.tbps / 1e6, 3),
               floor_share=round(floor / args.tbps / 1e9 / med["crop"], 5), moved_bytes=moved, equal_to_contract=equal,
               crop_torch_equal=bool(np.array_equal(got[1], toffs) and kc.same_bits(got[0], tp)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
