"""Times the KITTI PointPillars FROM RAW POINTS (configs/pointpillars/pointpillars_car_xyres16_points.py: md_voxelize ->
md_pp_pillar_encode -> md_pp_anchor_mask -> RPN -> merged heads -> post-processing) on a synthetic forward-facing cloud and prints ONE
JSON line.  Event-timed, three interleaved rounds of `--steps` as tools/pointpillars_step.py does; medians are reported.

  from_points_ms / pseudo_image_ms   (a) PointPillarsKITTIPoints.forward(points, offsets) against PointPillarsNet.forward on the canvas and
                                     the mask (a) produced -- the step the tree had before; the difference is the front end
  encoders                           (b) md_pp_pillar_encode against md_pillar_encode on the same voxels (F = 4, one layer: the fp32
                                     yardstick, which has neither the tenth feature nor the fp16 roundings -- a different function)
  anchor_mask                        (c) md_pp_anchor_mask against B calls of md_anchor_mask plus the voxel_num read-back
  launches                           each op's algorithmic bytes and its distance from the HBM floor (bytes / 8 TB/s / time, bench.py's
                                     formula).  The encoder's bytes: the canvas zero fill plus, per live row, its points, count and coors

The cloud is a MODELLING CHOICE of this tool, not a KITTI statistic: `--points` points per sample with 4 features (x, y, z,
reflectance), azimuth uniform within +-50 degrees of the x axis, the ground range log-uniform between 2 m and 70 m.

python tools/pointpillars_points_step.py [--batch 4] [--points 120000] [--steps 20] [--out profiles/pointpillars_kitti_points_step_b4.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_HBM_BPS = 8.0e12   # as bench.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kitti_cloud(batch, points_per_sample=120000, seed=0, rmin=2.0, rmax=70.0):
    """-> (points [N, 4] f32, offsets [batch + 1] i32), numpy; sample b has points_per_sample - 1000 b points (ragged)"""
    rng = np.random.default_rng(seed)
    parts = []
    for b in range(batch):
        n = points_per_sample - 1000 * b
        r = np.exp(rng.uniform(np.log(rmin), np.log(rmax), n))
        th = rng.uniform(-np.pi * 50 / 180, np.pi * 50 / 180, n)
        p = np.zeros((n, 4), np.float32)
        p[:, 0], p[:, 1] = r * np.cos(th), r * np.sin(th)
        p[:, 2] = rng.normal(-1.2, 0.6, n)
        p[:, 3] = rng.uniform(0, 1, n)
        parts.append(p)
    off = np.cumsum([0] + [len(p) for p in parts]).astype(np.int32)
    return np.concatenate(parts), off


def time_events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    from minddet.models import Config, build_detector
    from minddet_amd import det_ops, graphs

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", "pointpillars_car_xyres16_points.py"))
    model = build_detector(cfg.model, cfg.train_cfg, cfg.test_cfg).to(dev)
    inner = model.inner
    pts_h, off_h = kitti_cloud(args.batch, args.points, args.seed)
    points, offsets = torch.from_numpy(pts_h).to(dev), torch.from_numpy(off_h).to(dev)
    B = args.batch

    (dets, count), aux = model.forward(points, offsets, return_aux=True)
    canvas, mask = aux["pseudo_image"], aux["anchors_mask"]
    voxels, coors, num_points, voxel_num = (aux[k] for k in ("voxels", "coors", "num_points", "voxel_num"))
    dets_b, count_b = inner.forward(canvas, mask)
    same = bool(torch.equal(dets, dets_b) and torch.equal(count, count_b))
    same_mask = bool(torch.equal(mask, inner.anchors_mask_from_coors(coors, voxel_num)))

    # the fp32 yardstick of (b): the CenterPoint reader's one-layer form on the same voxels
    old_reader = graphs.PillarFeatureNet(num_input_features=4, num_filters=(64,), voxel_size=model.voxel_size, pc_range=model.pc_range).to(dev)
    rd = model.reader
    grid_xy = (model.grid_hw[1], model.grid_hw[0])
    fns = dict(
        from_points=lambda: model.forward(points, offsets),
        pseudo_image=lambda: inner.forward(canvas, mask),
        voxelize=lambda: det_ops.voxelize(points, offsets, model.voxel_size, model.pc_range, model.max_points, model.max_voxels),
        pp_pillar_encode=lambda: det_ops.pp_pillar_encode(voxels, num_points, coors, voxel_num, rd.packed, model.grid_hw, rd.voxel_size,
                                                          rd.offsets, out=canvas),
        pillar_encode_fp32=lambda: det_ops.pillar_encode(voxels, num_points, coors, voxel_num, old_reader.packed, model.grid_hw, old_reader.vx,
                                                         old_reader.vy, old_reader.x_offset, old_reader.y_offset),
        pp_anchor_mask=lambda: det_ops.anchors_mask_batched(coors, voxel_num, grid_xy, inner.anchors_bv, model.voxel_size, model.pc_range,
                                                            inner.anchor_area_threshold),
        anchor_mask_per_sample=lambda: inner.anchors_mask_from_coors(coors, voxel_num),
    )
    for fn in fns.values():
        fn()
    rounds = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            rounds[k].append(time_events(fn, args.steps))
    ms = {k: statistics.median(v) for k, v in rounds.items()}

    vn = [int(v) for v in voxel_num.cpu()]
    live = sum(vn)
    MP = model.max_points
    by = dict(voxelize=4.0 * points.numel() + 4.0 * (voxels.numel() + coors.numel() + num_points.numel()),
              pp_pillar_encode=2.0 * canvas.numel() + live * (16.0 * MP + 4 + 16 + 128),
              pp_anchor_mask=live * 16.0 + B * (3 * 4.0 * grid_xy[0] * grid_xy[1] * 2 + inner.anchors_bv.numel() * 4.0 + inner.anchors_bv.shape[0]))
    by["pillar_encode_fp32"] = by["pp_pillar_encode"]
    launches = [dict(op=k, mbytes=round(b / 1e6, 1), us=round(ms[k] * 1e3, 1), hbm_floor_us=round(b / PEAK_HBM_BPS * 1e6, 1),
                     frac_of_roofline=round(b / PEAK_HBM_BPS * 1e3 / ms[k], 3)) for k, b in by.items()]
    num = num_points.cpu().numpy()
    line = json.dumps(dict(
        metric="pointpillars_kitti_points_step", batch=B, steps=args.steps, points_per_sample=args.points, voxel_num=vn,
        mean_points_per_voxel=round(float(sum(num[b, :vn[b]].sum() for b in range(B)) / max(1, live)), 2),
        from_points_ms=round(ms["from_points"], 3), pseudo_image_ms=round(ms["pseudo_image"], 3),
        front_end_ms=round(ms["from_points"] - ms["pseudo_image"], 3),
        encoders=dict(pp_pillar_encode_us=round(ms["pp_pillar_encode"] * 1e3, 1), pillar_encode_fp32_us=round(ms["pillar_encode_fp32"] * 1e3, 1)),
        anchor_mask=dict(batched_us=round(ms["pp_anchor_mask"] * 1e3, 1), per_sample_with_readback_us=round(ms["anchor_mask_per_sample"] * 1e3, 1)),
        rounds_ms={k: [round(r, 4) for r in v] for k, v in rounds.items()}, launches=launches, same_detections=same, same_mask=same_mask,
        detections=[int(c) for c in count.cpu()]))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
