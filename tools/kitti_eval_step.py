"""Times the KITTI AP evaluation on the device (csrc/kittieval.hip) on a synthetic set of the size of the KITTI validation split -- 3 769
images, the class mix of tests/golden/kitti_eval_vectors.json, three classes, the full protocol (three difficulties, two overlap
levels, bbox / BEV / 3D + AOS) -- and prints ONE JSON line (also written to --out).

  images, gt_rows, dt_rows, pairs   the packed extents
  <op>_ms[metric]     flags, overlaps, match, sort, thresholds, stats: the median of three event-timed rounds of `steps` calls each, per
                      metric (flags and sort once: they do not depend on it; sort is torch.sort between match and thresholds)
  pack_ms             kitti_eval.pack_annos: host concatenation and the upload, wall time
  device_total_ms     get_official_eval_result(backend="device") on all images, wall time around the call, packing included
  host_subset_ms      get_official_eval_result (the host path) on the first --host-images images, wall time
  device_subset_ms    the device backend on the same subset
  host_ms_per_image   host_subset_ms / host_images: what the whole set would cost the host path at that rate is host_scaled_ms
                      (an extrapolation, not a measurement)
  subset_equal        the two backends print the same text on the subset apart from the aos lines, and the same dict within 1e-10
Not measured: real KITTI results (the detections here are jittered ground truth and strays), the host path on the whole set.

python tools/kitti_eval_step.py [--images 3769] [--host-images 200] [--steps 5] [--out profiles/kitti_eval_device.json]
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
from minddet_amd import det_ops  # noqa: E402
from minddet_amd import kitti_eval as ke  # noqa: E402

DEV = "cuda:0"


def class_mix():
    """names and their frequencies over the fixture's ground truth, and its mean rows per image"""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "kitti_eval_vectors.json")))
    names = [n for c in gold["cases"] for a in c["gt"] for n in a["name"]]
    uniq, cnt = np.unique(names, return_counts=True)
    return uniq.tolist(), cnt / cnt.sum(), len(names) / sum(len(c["gt"]) for c in gold["cases"])


def synthetic(rng, n_img, names, freq, mean_rows):
    gts, dts = [], []
    for _ in range(n_img):
        n = int(rng.poisson(mean_rows))
        loc = np.stack([rng.uniform(-15, 15, n), np.full(n, 1.6), rng.uniform(5, 45, n)], 1)
        dims = np.stack([rng.uniform(3.2, 4.6, n), rng.uniform(1.4, 1.7, n), rng.uniform(1.5, 1.8, n)], 1)
        u, half = 600 + 700 * loc[:, 0] / loc[:, 2], 700 * 2.0 / loc[:, 2]
        bbox = np.stack([u - half, 180 - 40 - 600 / loc[:, 2], u + half, 180 + 600 / loc[:, 2]], 1)
        g = dict(name=rng.choice(names, n, p=freq), bbox=bbox, location=loc, dimensions=dims, rotation_y=rng.uniform(-3, 3, n),
                 occluded=rng.integers(0, 3, n), truncated=rng.choice([0.0, 0.2, 0.4], n), alpha=rng.uniform(-3, 3, n))
        keep = (g["name"] != "DontCare") & (rng.random(n) < 0.85)                      # detections: most objects found, jittered; a few strays
        k, s = int(keep.sum()), int(rng.integers(0, 3))
        d = {key: np.concatenate([g[key][keep], g[key][rng.integers(0, max(n, 1), s)] if n else g[key][:0]]) for key in g}
        d["location"] = d["location"] + rng.normal(0, 0.15, d["location"].shape) + np.concatenate([np.zeros((k, 3)), rng.uniform(3, 8, (len(d["name"]) - k, 3))])
        d["bbox"] = d["bbox"] + rng.normal(0, 2.0, d["bbox"].shape) + np.concatenate([np.zeros((k, 4)), np.full((len(d["name"]) - k, 4), 150.0)])
        d["rotation_y"] = d["rotation_y"] + rng.normal(0, 0.05, len(d["name"]))
        d["alpha"] = d["alpha"] + rng.normal(0, 0.1, len(d["name"]))
        d["name"] = np.where(d["name"] == "DontCare", "Car", d["name"])
        d["score"] = rng.uniform(0.05, 1.0, len(d["name"]))
        gts.append(g)
        dts.append(d)
    return gts, dts


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
    ap.add_argument("--images", type=int, default=3769)
    ap.add_argument("--host-images", type=int, default=200)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kitti_eval_device.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kitti_eval_step: needs the GPU (a time taken anywhere else says nothing)")
    names, freq, mean_rows = class_mix()
    gt, dt = synthetic(np.random.default_rng(args.seed), args.images, names, freq, mean_rows)
    classes = [0, 1, 2]
    mo = ke._MIN_OVERLAPS_FULL[:, :, classes]
    pack_ms, p = wall(lambda: ke.pack_annos(gt, dt, device=DEV))
    idx = torch.tensor(classes, device=DEV)
    res = dict(metric="kitti_eval_device", images=args.images, classes=3, difficulties=3, levels=int(mo.shape[0]), gt_rows=int(p.gt_box.shape[0]),
               dt_rows=int(p.dt_box.shape[0]), pairs=int(p.pairs), steps=args.steps, pack_ms=round(pack_ms, 3))
    rounds = {}

    def timed(key, fn):
        fn()
        torch.cuda.synchronize()
        rounds[key] = [time_calls(fn, args.steps) for _ in range(3)]
        return fn()

    flags = timed("flags", lambda: det_ops.kitti_eval_flags(p.gt_box, p.gt_occ, p.gt_trunc, p.gt_valid[idx], p.dt_box, p.dt_same[idx], False))
    for metric in (0, 1, 2):
        min_ov = torch.from_numpy(np.ascontiguousarray(mo[:, metric, :].T)).to(DEV)
        g, d = (p.gt_box, p.dt_box) if metric == 0 else (p.gt_cam, p.dt_cam)
        offs = (p.gt_off, p.dt_off, p.ov_off, min_ov)
        ov = timed(f"overlaps[{metric}]", lambda: det_ops.kitti_eval_overlaps(p.gt_off, p.dt_off, p.ov_off, g, d, metric, p.pairs))
        matched = timed(f"match[{metric}]", lambda: det_ops.kitti_eval_match(ov, flags[0], flags[1], p.dt_score, *offs))
        ordered = timed(f"sort[{metric}]", lambda: torch.sort(matched, dim=-1, descending=True).values)
        thr, nth = timed(f"thresholds[{metric}]", lambda: det_ops.kitti_eval_thresholds(ordered, flags[2]))
        timed(f"stats[{metric}]", lambda: det_ops.kitti_eval_stats(ov, flags[0], flags[1], p.dt_score, *offs, thr, nth, p.gt_box, p.gt_dc, p.dt_box, p.gt_alpha,
                                                                     p.dt_alpha, metric, metric == 0))
        res[f"nthresh[{metric}]"] = nth.cpu().numpy().reshape(-1).tolist()
    for key, v in rounds.items():
        res[key + "_ms"] = round(statistics.median(v), 4)
        res[key + "_rounds_ms"] = [round(t, 4) for t in v]
    res["ops_sum_ms"] = round(sum(statistics.median(v) for v in rounds.values()), 3)
    ke.get_official_eval_result(gt[:8], dt[:8], classes, backend="device")
    res["device_total_ms"] = round(wall(lambda: ke.get_official_eval_result(gt, dt, classes, backend="device"))[0], 2)
    n = min(args.host_images, args.images)
    host_ms, (h_text, h_out) = wall(lambda: ke.get_official_eval_result(gt[:n], dt[:n], classes))
    dev_ms, (d_text, d_out) = wall(lambda: ke.get_official_eval_result(gt[:n], dt[:n], classes, backend="device"))
    no_aos = lambda t: [l for l in t.splitlines() if not l.startswith("aos")]
    res.update(host_images=n, host_subset_ms=round(host_ms, 1), device_subset_ms=round(dev_ms, 2), host_ms_per_image=round(host_ms / n, 2),
               host_scaled_ms=round(host_ms / n * args.images, 0), host_scaled_is_extrapolated=True,
               subset_equal=bool(no_aos(h_text) == no_aos(d_text) and set(h_out) == set(d_out) and all(abs(h_out[k] - d_out[k]) <= 1e-10 for k in h_out)),
               car_3d_moderate_r40=round(d_out["Car_3d/moderate_R40"], 4))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
