"""Times the KITTI PointPillars training augmentation (det_ops.pc_noise_per_object / pc_augment_points / pc_augment_boxes =
csrc/pcaug.hip) and the whole graphs.PointPillarsKITTIPoints.train_example at the shape of
configs/pointpillars/pointpillars_car_xyres16_train.py -- B = 4, 120 000 points per sample, 15 ground-truth boxes + 10 sampled ones per
sample (G = 25, R = 10 remove boxes, the sampled objects' points in front), T = 100 tries -- and prints ONE JSON line (also written
to --out).

  noise_ms / points_ms / boxes_ms / train_example_ms (+ *_rounds_ms)
                      median / each of three event-timed rounds of `steps` calls, the rounds of all timed things interleaved
  points_floor_us / points_floor_share
                      the points pass's least traffic (every point read once and written once, 16 bytes each way, plus the owner,
                      4 bytes) / --tbps (default 6.0 TB/s), and that time as a fraction of points_ms
  noise_bytes / boxes_bytes and their floors likewise (draws read once, outputs written once)
  torch_points_ms     baseline (a): the points pass as torch device ops in float64 without a host read (sample by bucketize, [N, G + R]
                      inside tests, first-owner by argmax, transform, compaction by cumsum + scatter into a dummy-row buffer).  The
                      sequential noise_per_object has no such twin (each box depends on where the earlier ones ended up): not timed.
  host_contract_ms    baseline (b): tests/pcaug_contract.py on the host for the B samples, including the copy of the points to the host
                      and of the result back: what a training step pays today for augmenting off the device
  equal_to_contract   the device result meets the conditions of tests/test_pc_augment_gpu.py against the contract on sample 0

python tools/pointpillars_augment_step.py [--steps 20] [--out profiles/pointpillars_augment_step_b4.json]
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
from minddet_amd import det_ops  # noqa: E402
from tests import pcaug_contract as pc  # noqa: E402

DEV = "cuda:0"


def scene(B, n, G0, R, seed):
    rng = np.random.default_rng(seed)
    G = G0 + R
    boxes = np.zeros((B, G, 7), np.float32)
    for b in range(B):
        cells = [(x, y) for x in np.arange(6, 66, 6.0) for y in np.arange(-36, 37, 8.0)]
        for g, k in enumerate(rng.permutation(len(cells))[:G]):
            boxes[b, g] = (cells[k][0] + rng.uniform(-1, 1), cells[k][1] + rng.uniform(-1, 1), rng.uniform(-1.8, -1.2), 1.6, 3.9, 1.56,
                           rng.uniform(-np.pi, np.pi))
    rem = boxes[:, G0:].copy()
    front = 200 * R
    pts = []
    for b in range(B):
        own = boxes[b, G0 + rng.integers(0, R, front), :3] + rng.uniform(-0.7, 0.7, (front, 3)) + (0, 0, 0.8)
        bg = np.stack([rng.uniform(0, 69, n - front), rng.uniform(-39, 39, n - front), rng.uniform(-2.5, 0.5, n - front)], 1)
        pts.append(np.concatenate([np.concatenate([own, bg]), rng.uniform(0, 1, (n, 1))], 1).astype(np.float32))
    return dict(points=np.concatenate(pts), offsets=np.arange(0, (B + 1) * n, n, dtype=np.int32), boxes=boxes,
                count=np.full(B, G, np.int32), valid=np.ones((B, G), np.uint8), classes=np.ones((B, G), np.int32), rem=rem,
                rem_count=np.full(B, R, np.int32), rem_from=np.full(B, front, np.int32))


def time_calls(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_points(points, offsets, boxes, rem, valid, tf, glob, rem_from):
    """baseline (a): the points pass as torch device ops, float64, no host read"""
    N, (B, G), R = points.shape[0], boxes.shape[:2], rem.shape[1]
    idx = torch.arange(N, device=points.device)
    b = torch.bucketize(idx, offsets[1:].long(), right=True).clamp_(max=B - 1)
    allb = torch.cat([boxes, rem], 1).double()[b]                                       # [N, G + R, 7]
    p = points.double()
    d = p[:, None, :3] - allb[..., :3]
    c, s = torch.cos(allb[..., 6]), torch.sin(allb[..., 6])
    lx, ly = d[..., 0] * c - d[..., 1] * s, d[..., 0] * s + d[..., 1] * c
    inside = (lx.abs() < allb[..., 3] / 2) & (ly.abs() < allb[..., 4] / 2) & (d[..., 2] > 0) & (d[..., 2] < allb[..., 5])
    late = (idx - offsets[b].long()) >= rem_from[b].long()
    drop = late & inside[:, G:].any(1)
    obj = inside[:, :G] & (valid[b] != 0)
    has, own = obj.any(1), obj.to(torch.uint8).argmax(1)
    t, cen = tf[b, own], boxes.double()[b, own]
    q = p[:, :3] - cen[:, :3]
    ct, st = torch.cos(t[:, 3]), torch.sin(t[:, 3])
    moved = torch.stack([q[:, 0] * ct + q[:, 1] * st, -q[:, 0] * st + q[:, 1] * ct, q[:, 2]], 1) + cen[:, :3] + t[:, :3]
    xyz = torch.where(has[:, None], moved, p[:, :3])
    g = glob[b]
    y = torch.where(g[:, 0] != 0, -xyz[:, 1], xyz[:, 1])
    cg, sg = torch.cos(g[:, 1]), torch.sin(g[:, 1])
    out = torch.stack([(xyz[:, 0] * cg + y * sg) * g[:, 2] + g[:, 3], (-xyz[:, 0] * sg + y * cg) * g[:, 2] + g[:, 4],
                       xyz[:, 2] * g[:, 2] + g[:, 5], p[:, 3]], 1).float()
    keep = ~drop
    pos = torch.where(keep, torch.cumsum(keep, 0) - 1, torch.full_like(idx, N))
    buf = torch.zeros((N + 1, 4), dtype=torch.float32, device=points.device)
    buf.scatter_(0, pos[:, None].expand(-1, 4), out)
    return buf[:N], torch.where(drop, -2, torch.where(has, own, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tbps", type=float, default=6.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointpillars_augment_step_b4.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointpillars_augment_step: needs the GPU (a time taken anywhere else says nothing)")
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", "pointpillars_car_xyres16_train.py"))
    # the reference's own defaults for the per-object global rotation (the yaml switches it off): the v2 form is the dearer one
    train_cfg = dict(cfg.train_cfg, augment=dict(cfg.train_cfg["augment"], global_random_rot_range=[0.78, 2.35]))
    model = build_detector(dict(cfg.model), train_cfg, cfg.test_cfg).to(DEV)
    aug = model.augment_op()
    B, n, G0, R = args.batch, args.points, 15, 10
    s = scene(B, n, G0, R, args.seed)
    d = {k: torch.from_numpy(v).to(DEV) for k, v in s.items()}
    draws = aug.draw(d["boxes"], d["count"], torch.Generator(device=DEV).manual_seed(args.seed))
    sampled = dict(remove_boxes=d["rem"], remove_count=d["rem_count"], remove_from=d["rem_from"])
    N, G, T = B * n, G0 + R, aug.num_try

    def noise():
        return det_ops.pc_noise_per_object(d["boxes"], d["count"], d["valid"], draws["loc"], draws["rot"], draws["grot"])

    sel, tf, moved = noise()

    def points():
        return det_ops.pc_augment_points(d["points"], d["offsets"], d["boxes"], d["count"], d["valid"], tf, draws["glob"], d["rem"],
                                         d["rem_count"], d["rem_from"])

    def boxes():
        return det_ops.pc_augment_boxes(moved, d["count"], d["valid"], d["classes"], draws["glob"], aug.bv_range)

    def example():
        return model.train_example(d["points"], d["offsets"], d["boxes"], d["classes"], d["count"], draws=draws, sampled=sampled)

    def torch_twin():
        return torch_points(d["points"], d["offsets"], d["boxes"], d["rem"], d["valid"], tf, draws["glob"], d["rem_from"])

    timed = dict(noise=noise, points=points, boxes=boxes, train_example=example, torch_points=torch_twin)
    for fn in timed.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in timed}
    for _ in range(3):
        for k, fn in timed.items():
            rounds[k].append(time_calls(fn, args.steps))
    med = {k: statistics.median(v) for k, v in rounds.items()}

    host, tf_np = [], tf.cpu().numpy()
    for _ in range(3):
        t0 = time.perf_counter()
        p_host = d["points"].cpu().numpy()
        outs = []
        for b in range(B):
            sel_b, tf_b, moved_b = pc.noise_per_object(s["boxes"][b], G, s["valid"][b], draws["loc"][b].cpu().numpy(), draws["rot"][b].cpu().numpy(),
                                                       draws["grot"][b].cpu().numpy())
            o = pc.augment_points(p_host[b * n:(b + 1) * n], s["boxes"][b], G, s["valid"][b], tf_b, draws["glob"][b].cpu().numpy(), s["rem"][b], R,
                                  int(s["rem_from"][b]))
            pc.augment_boxes(moved_b, G, s["valid"][b], s["classes"][b], draws["glob"][b].cpu().numpy(), aug.bv_range)
            outs.append(o["points"])
        back = torch.from_numpy(np.concatenate(outs)).to(DEV)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
    del back
    got_p, got_o, got_own = (t.cpu().numpy() for t in points())
    sel0, tf0, _ = pc.noise_per_object(s["boxes"][0], G, s["valid"][0], draws["loc"][0].cpu().numpy(), draws["rot"][0].cpu().numpy(),
                                       draws["grot"][0].cpu().numpy())
    want = pc.augment_points(s["points"][:n], s["boxes"][0], G, s["valid"][0], tf0, draws["glob"][0].cpu().numpy(), s["rem"][0], R,
                             int(s["rem_from"][0]))
    k = len(want["points"])
    step = np.spacing(np.maximum(np.abs(want["points"][:, :3]), np.float32(1e-30)))
    equal = bool(np.array_equal(sel.cpu().numpy()[0], sel0) and np.array_equal(got_own[:n], want["owner"]) and int(got_o[1]) == k and
                 (np.abs(got_p[:k, :3].astype(np.float64) - want["points"][:, :3]) <= step).all() and
                 np.abs(tf_np[0] - tf0).max() <= 4 * np.spacing(np.abs(tf0).max()))
    tw_p, tw_own = torch_twin()
    twin_equal = bool(torch.equal(tw_own.int().cpu(), torch.from_numpy(got_own)) and
                      (tw_p.cpu() - torch.from_numpy(got_p)).abs().max().item() <= 1e-5)

    pbytes = N * (16 + 16 + 4)
    nbytes = B * G * T * 5 * 8 + B * G * (7 * 4 + 4 + 4 * 8 + 7 * 4)
    bbytes = B * G * (7 * 4 * 2 + 4 * 2 + 1) + B * 52

    def floor(nb, ms):
        return round(nb / args.tbps / 1e6, 3), round(nb / args.tbps / 1e9 / ms, 5)

    res = dict(metric="pointpillars_augment_step", config="pointpillars_car_xyres16_train (per-object global rotation on)", batch=B,
               points_per_sample=n, boxes_per_sample=G, remove_boxes=R, tries=T, steps=args.steps,
               kept_points=int(got_o[-1]), selected_first_try=int((sel == 0).sum()), selected_none=int((sel < 0).sum()),
               tbps=args.tbps)
    for key in timed:
        res[key + "_ms"] = round(med[key], 4)
        res[key + "_rounds_ms"] = [round(t, 4) for t in rounds[key]]
    for key, nb in (("noise", nbytes), ("points", pbytes), ("boxes", bbytes)):
        res[key + "_bytes"] = nb
        res[key + "_floor_us"], res[key + "_floor_share"] = floor(nb, med[key])
    res.update(ops_sum_ms=round(med["noise"] + med["points"] + med["boxes"], 4),
               torch_points_over_points=round(med["torch_points"] / med["points"], 2), torch_points_equal=twin_equal,
               torch_noise_ms=None, torch_noise_missing="sequential over the boxes of a sample: no torch twin without a host loop; not timed",
               host_contract_ms=round(statistics.median(host), 2), host_contract_rounds_ms=[round(t, 2) for t in host],
               host_is="tests/pcaug_contract.py (vectorised numpy float64) for the B samples plus the copy of the points to the host and of the "
                       "result back; not the reference's numba loops, which are not part of this repository",
               equal_to_contract=equal)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
