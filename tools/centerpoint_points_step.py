"""Times the CenterPoint-PP detector FROM RAW POINTS (configs/centerpoint/centerpoint_pp_nusc_points.py: md_voxelize -> md_pillar_encode
-> RPN neck -> CenterHead -> post-processing) on a synthetic sweep-like cloud and prints ONE JSON line:

  from_points_ms        (a) PillarDetector.forward(points, offsets)
  pseudo_image_ms       (b) PointPillars.forward on the canvas (a) produced -- the step the tree had before; (a) - (b) is the front end
  launches              (c) md_voxelize and md_pillar_encode alone: algorithmic bytes (inputs read once, outputs written once), time and
                        frac_of_roofline = bytes / 8 TB/s / time (bench.py's formula; neither op has MFMA work)
  torch_front_end_ms    (d) the same front end as a plain torch-on-device composition (unique / stable sort / index_put / F.linear):
                        what a user could write without the two kernels; its voxel count is checked against (a)'s
  same_detections       the step from points gives bit-identical (dets, count) to (b)
(a), (b) and (d) are interleaved in each of three rounds on the same box; the medians are reported.

The cloud is a MODELLING CHOICE of this tool, not a nuScenes statistic: `--points` points per sample with 5 features (x, y, z,
intensity, sweep time), uniform in azimuth, the ground range log-uniform between 1 m and `--rmax` (the areal density falls with the
square of the range, as a spinning sensor's does), so cells near the sensor hold far more than max_points_in_voxel points and far
cells hold 1-3.

python tools/centerpoint_points_step.py [--batch 4] [--points 260000] [--steps 10] [--out profiles/centerpoint_points_step_b4.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_HBM_BPS = 8.0e12   # as bench.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sweep_cloud(batch, points_per_sample=260000, seed=0, rmax=32.0, features=5):
    """-> (points [N, features] f32, offsets [batch + 1] i32), numpy; sample b has points_per_sample - 1000 b points (ragged)"""
    rng = np.random.default_rng(seed)
    parts = []
    for b in range(batch):
        n = points_per_sample - 1000 * b
        r = np.exp(rng.uniform(0.0, np.log(rmax), n))
        th = rng.uniform(0, 2 * np.pi, n)
        p = np.zeros((n, features), np.float32)
        p[:, 0], p[:, 1] = r * np.cos(th), r * np.sin(th)
        p[:, 2] = rng.normal(-1.0, 0.8, n)
        p[:, 3] = rng.uniform(0, 1, n)
        if features > 4:
            p[:, 4] = rng.integers(0, 10, n) * 0.05
        parts.append(p)
    off = np.cumsum([0] + [len(p) for p in parts]).astype(np.int32)
    return np.concatenate(parts), off


def torch_front_end(points, offsets_host, model):
    """the front end from torch ops on the device -> (canvas [B, H, W, 64] bf16, voxel_num list).  Same semantics as the two kernels
    (first-point voxel order, the max_voxels cut, the first max_points points by index, padded rows in the maximum)."""
    dev = points.device
    rd, MP, MV = model.reader, model.max_points, model.max_voxels
    H, W = model.grid_hw
    lo = torch.tensor(model.pc_range[:3], dtype=torch.float32, device=dev)
    vs = torch.tensor(model.voxel_size, dtype=torch.float32, device=dev)
    B = len(offsets_host) - 1
    canvas = torch.zeros((B, H, W, 64), dtype=torch.bfloat16, device=dev)
    pk = rd.packed
    counts = []
    for b in range(B):
        p = points[offsets_host[b]:offsets_host[b + 1]]
        c = torch.floor((p[:, :3] - lo) / vs)
        ok = torch.isfinite(p[:, :3]).all(1) & (c >= 0).all(1) & (c[:, 0] < W) & (c[:, 1] < H) & (c[:, 2] < 1)
        p, c = p[ok], c[ok].long()
        cid = c[:, 1] * W + c[:, 0]
        uniq, inv = torch.unique(cid, return_inverse=True)
        idx = torch.arange(len(cid), device=dev)
        first = torch.full((len(uniq),), len(cid), device=dev, dtype=torch.long).scatter_reduce(0, inv, idx, "amin")
        rank = torch.empty_like(first)
        rank[torch.argsort(first, stable=True)] = torch.arange(len(uniq), device=dev)
        vox = rank[inv]
        keep = vox < MV
        p, vox = p[keep], vox[keep]
        order = torch.argsort(vox, stable=True)
        p, vox = p[order], vox[order]
        cnt = torch.bincount(vox, minlength=MV)[:MV]
        start = torch.cumsum(cnt, 0) - cnt
        slot = torch.arange(len(vox), device=dev) - start[vox]
        take = slot < MP
        voxels = torch.zeros((MV, MP, p.shape[1]), dtype=torch.float32, device=dev)
        voxels.index_put_((vox[take], slot[take]), p[take])
        num = torch.clamp(cnt, max=MP)
        cell = torch.zeros((MV,), dtype=torch.long, device=dev)
        cell[rank[rank < MV]] = uniq[rank < MV]
        live = num > 0
        mean = voxels[:, :, :3].sum(1, keepdim=True) / num.clamp(min=1).view(-1, 1, 1).float()
        cx, cy = (cell % W).float().view(-1, 1), (cell // W).float().view(-1, 1)
        f = torch.cat([voxels, voxels[:, :, :3] - mean, (voxels[:, :, 0] - (cx * rd.vx + rd.x_offset)).unsqueeze(2),
                       (voxels[:, :, 1] - (cy * rd.vy + rd.y_offset)).unsqueeze(2)], 2)
        f = f * (torch.arange(MP, device=dev).view(1, MP) < num.view(-1, 1)).unsqueeze(2)
        x = torch.relu(F.linear(f, pk.w1, pk.b1))
        m = x.max(1).values
        if pk.w2 is not None:
            x = torch.relu(F.linear(torch.cat([x, m.unsqueeze(1).expand(-1, MP, -1)], 2), pk.w2, pk.b2))
            m = x.max(1).values
        canvas[b].view(H * W, 64).index_put_((cell[live],), m[live].to(torch.bfloat16))
        counts.append(int(live.sum()))       # (the one host read of this composition, after its last launch)
    return canvas, counts


def time_events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def wall(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    from minddet.models import Config, build_detector
    from minddet_amd import det_ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--points", type=int, default=260000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rmax", type=float, default=32.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc_points.py"))
    model = build_detector(cfg.model, cfg.train_cfg, cfg.test_cfg).to(dev)
    pts_h, off_h = sweep_cloud(args.batch, args.points, args.seed, args.rmax)
    points, offsets = torch.from_numpy(pts_h).to(dev), torch.from_numpy(off_h).to(dev)
    off_list = [int(v) for v in off_h]
    B = args.batch

    (dets, count), aux = model.forward(points, offsets, return_aux=True)
    canvas = aux["pseudo_image"]
    dets_b, count_b = model.detector.forward(canvas)
    same = bool(torch.equal(dets, dets_b) and torch.equal(count, count_b))
    t_canvas, t_counts = torch_front_end(points, off_list, model)
    voxel_num = [int(v) for v in aux["voxel_num"].cpu()]
    canvas_diff = float((t_canvas.float() - canvas.float()).abs().max())

    a = lambda: model.forward(points, offsets)
    b = lambda: model.detector.forward(canvas)
    d = lambda: torch_front_end(points, off_list, model)
    fe = lambda: model.pseudo_image(points, offsets)
    for fn in (a, b, d, fe):
        fn()
    ra, rb, rd_, rf = [], [], [], []
    for _ in range(3):
        ra.append(wall(a, args.steps))
        rb.append(wall(b, args.steps))
        rd_.append(wall(d, max(1, args.steps // 5)))
        rf.append(wall(fe, args.steps))
    ms_a, ms_b, ms_d, ms_f = (statistics.median(r) for r in (ra, rb, rd_, rf))

    vox = aux["voxels"], aux["coors"], aux["num_points"], aux["voxel_num"]
    t_vox = statistics.median(time_events(lambda: det_ops.voxelize(points, offsets, model.voxel_size, model.pc_range, model.max_points,
                                                                   model.max_voxels), args.steps) for _ in range(3))
    t_enc = statistics.median(time_events(lambda: model.backbone(model.reader, vox[0], vox[1], vox[2], vox[3], model.grid_hw), args.steps)
                              for _ in range(3))
    by_vox = 4.0 * points.numel() + 4.0 * (vox[0].numel() + vox[1].numel() + vox[2].numel())
    by_enc = 4.0 * (vox[0].numel() + vox[1].numel() + vox[2].numel()) + 2.0 * canvas.numel()
    launches = [dict(op=n, mbytes=round(by / 1e6, 1), us=round(t * 1e3, 1), hbm_floor_us=round(by / PEAK_HBM_BPS * 1e6, 1),
                     frac_of_roofline=round(by / PEAK_HBM_BPS * 1e3 / t, 3)) for n, by, t in (("md_voxelize", by_vox, t_vox),
                                                                                            ("md_pillar_encode", by_enc, t_enc))]
    num = aux["num_points"].cpu().numpy()
    line = json.dumps(dict(
        metric="centerpoint_points_step", batch=B, steps=args.steps, points_per_sample=args.points, voxel_num=voxel_num,
        full_voxels=[int((num[i] == model.max_points).sum()) for i in range(B)],
        mean_points_per_voxel=round(float(num.sum() / max(1, sum(voxel_num))), 2),
        from_points_ms=round(ms_a, 3), pseudo_image_ms=round(ms_b, 3), front_end_ms=round(ms_a - ms_b, 3), front_end_alone_ms=round(ms_f, 3),
        torch_front_end_ms=round(ms_d, 3), speedup_over_torch=round(ms_d / ms_f, 1),
        rounds_ms=dict(from_points=[round(r, 3) for r in ra], pseudo_image=[round(r, 3) for r in rb], torch=[round(r, 3) for r in rd_],
                       front_end=[round(r, 3) for r in rf]),
        launches=launches, same_detections=same, detections=[int(c) for c in count.cpu()], torch_voxel_num=t_counts,
        torch_canvas_max_abs_diff=round(canvas_diff, 5)))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
