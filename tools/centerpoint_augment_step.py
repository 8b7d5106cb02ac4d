"""Times the CenterPoint training input (det_ops.cp_aug_count_points / cp_aug_select / cp_aug_points / cp_aug_boxes = csrc/cpaug.hip)
and the chain of graphs.PillarDetector from points to gradient, with and without the augmentation, at the shape of
configs/centerpoint/centerpoint_pp_nusc_train.py -- B = 4, 260 000 points per sample (ten sweeps), G = 60 ground-truth rows and S = 40
sampler candidates in four groups per sample, 50 points per candidate -- and prints ONE JSON line (also written to --out).

  count_ms / select_ms / points_ms / boxes_ms / chain_augmented_ms / chain_plain_ms (+ *_rounds_ms)
                      median / each of three event-timed rounds of `steps` calls, the rounds of all timed things interleaved
  chain_augmented     PillarDetector.train_loss(grad=True): the four ops, md_voxelize (30 000 voxels), md_pillar_encode, neck, head,
                      md_cp_assign_targets, md_cp_loss_grad
  chain_plain         the same chain on the raw points and the given ground truth (no augmentation): targets_op + loss(grad=True)
  *_bytes / *_floor_us / *_floor_share
                      each op's algorithmic traffic (count: every point's x, y, z read once, 12 bytes, and the boxes; points: every
                      row read once and written once, 20 bytes each way; select and boxes: the boxes and masks in, the outputs out)
                      / --tbps (default 6.0 TB/s), and that time as a fraction of the op's time
  equal_to_contract   the device result meets the conditions of tests/test_cp_augment_gpu.py against tests/cpaug_contract.py on sample 0

python tools/centerpoint_augment_step.py [--steps 20] [--out profiles/centerpoint_augment_step_b4.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from minddet.models import Config, build_detector  # noqa: E402
from minddet_amd import det_ops  # noqa: E402
from tests import cpaug_contract as cc  # noqa: E402

DEV = "cuda:0"


def scene(B, n, G, S, per, seed):
    rng = np.random.default_rng(seed)

    def boxes(k, spread):
        b = np.zeros((B, k, 9), np.float32)
        b[..., 0], b[..., 1], b[..., 2] = rng.uniform(-spread, spread, (B, k)), rng.uniform(-spread, spread, (B, k)), rng.uniform(-1.5, -0.5, (B, k))
        b[..., 3], b[..., 4], b[..., 5] = rng.uniform(0.6, 2.6, (B, k)), rng.uniform(0.6, 7.0, (B, k)), rng.uniform(1.0, 3.0, (B, k))
        b[..., 6:8], b[..., 8] = rng.uniform(-5, 5, (B, k, 2)), rng.uniform(-np.pi, np.pi, (B, k))
        return b
    gt, cand = boxes(G, 50.0), boxes(S, 45.0)
    pts = []
    for b in range(B):
        k = n // 20                                           # one point in twenty on an object
        own = gt[b, rng.integers(0, G, k), :3] + rng.uniform(-0.8, 0.8, (k, 3))
        r, a = 60 * np.sqrt(rng.uniform(0, 1, n - k)), rng.uniform(0, 2 * np.pi, n - k)
        bg = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-3.0, 1.0, n - k)], 1)
        xyz = np.concatenate([own, bg])[rng.permutation(n)]
        pts.append(np.concatenate([xyz, rng.uniform(0, 1, (n, 1)), rng.uniform(0, 0.5, (n, 1))], 1).astype(np.float32))
    cand_points = np.concatenate([rng.uniform(-0.4, 0.4, (B * S * per, 3)), rng.uniform(0, 1, (B * S * per, 2))], 1).astype(np.float32)
    return dict(points=np.concatenate(pts), offsets=np.arange(0, (B + 1) * n, n, dtype=np.int32), gt_boxes=gt, gt_count=np.full(B, G, np.int32),
                gt_classes=(1 + rng.integers(0, 10, (B, G))).astype(np.int32), cand_boxes=cand, cand_count=np.full(B, S, np.int32),
                cand_classes=(1 + rng.integers(0, 10, (B, S))).astype(np.int32), cand_group=np.tile(np.arange(S, dtype=np.int32) * 4 // S, (B, 1)),
                cand_points=cand_points, cand_offsets=np.arange(0, B * S * per + 1, per, dtype=np.int32))


def time_calls(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--points", type=int, default=260000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tbps", type=float, default=6.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "centerpoint_augment_step_b4.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("centerpoint_augment_step: needs the GPU (a time taken anywhere else says nothing)")
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc_train.py"))
    train_cfg = dict(cfg.train_cfg, augment=dict(cfg.train_cfg["augment"], min_points_in_gt=5, global_translate_std=0.2))
    model = build_detector(dict(cfg.model), train_cfg, cfg.test_cfg).to(DEV)
    aug = model.augment_op()
    B, n, G, S, per = args.batch, args.points, 60, 40, 50
    s = scene(B, n, G, S, per, args.seed)
    d = {k: torch.from_numpy(v).to(DEV) for k, v in s.items()}
    glob = aug.draw(B, torch.Generator(device=DEV).manual_seed(args.seed))
    sampled = dict(points=d["cand_points"], offsets=d["cand_offsets"], boxes=d["cand_boxes"], classes=d["cand_classes"], group=d["cand_group"],
                   count=d["cand_count"])
    N, Ns = B * n, B * S * per

    def count():
        return det_ops.cp_aug_count_points(d["points"], d["offsets"], d["gt_boxes"], d["gt_count"], aug.min_points_in_gt)

    counts, keep = count()

    def select():
        return det_ops.cp_aug_select(d["gt_boxes"], d["gt_count"], keep, d["cand_boxes"], d["cand_count"], d["cand_group"])

    accept = select()

    def points():
        return det_ops.cp_aug_points(d["points"], d["offsets"], glob, d["cand_points"], d["cand_offsets"], d["cand_boxes"], accept)

    def boxes():
        return det_ops.cp_aug_boxes(d["gt_boxes"], d["gt_classes"], d["gt_count"], keep, glob, aug.bv_range, d["cand_boxes"], d["cand_classes"], accept)

    def chain_augmented():
        return model.train_loss(d["points"], d["offsets"], d["gt_boxes"], d["gt_classes"], d["gt_count"], draws=glob, sampled=sampled, grad=True)

    def chain_plain():
        return model.loss(d["points"], d["offsets"], model.targets_op()(d["gt_boxes"], d["gt_classes"]), grad=True)

    timed = dict(count=count, select=select, points=points, boxes=boxes, chain_augmented=chain_augmented, chain_plain=chain_plain)
    for fn in timed.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in timed}
    for _ in range(3):
        for k, fn in timed.items():
            rounds[k].append(time_calls(fn, args.steps))
    med = {k: statistics.median(v) for k, v in rounds.items()}

    # sample 0 against the contract, by the rule of tests/test_cp_augment_gpu.py
    c0 = cc.count_points(s["points"][:n], s["gt_boxes"][0], G, aug.min_points_in_gt)
    got_counts, got_keep, got_acc = counts.cpu().numpy()[0], keep.cpu().numpy()[0], accept.cpu().numpy()[0]
    equal = bool(((got_counts >= c0["lo"]) & (got_counts <= c0["hi"])).all() and np.array_equal(got_keep[c0["keep_decided"]], c0["keep"][c0["keep_decided"]]))
    if equal and np.array_equal(got_keep, c0["keep"]):
        want_acc = cc.select(s["gt_boxes"][0], G, c0["keep"], s["cand_boxes"][0], S, s["cand_group"][0])
        want = cc.augment_points(s["points"][:n], glob[0].cpu().numpy(), s["cand_points"], s["cand_offsets"][:S + 1], s["cand_boxes"][0], want_acc)
        p, o = (t.cpu().numpy() for t in points())
        k = len(want["points"])
        step = np.spacing(np.maximum(np.abs(want["points"][:, :3]), np.float32(1e-30)))
        equal = bool(np.array_equal(got_acc, want_acc) and int(o[1]) == k and
                     (np.abs(p[:k, :3].astype(np.float64) - want["points"][:, :3]) <= step).all() and np.array_equal(p[:k, 3:], want["points"][:, 3:]))
    out_boxes, out_cls, out_count = boxes()

    W = (G + S + 63) // 64
    nbytes = dict(count=N * 12 + B * G * (36 + 4 + 4 + 1), select=B * (G + S) * 36 + B * G + B * S * (4 + 1) + B * S * W * 16,
                  points=(N + Ns) * 20 + int(points()[1][-1]) * 20 + B * S * 37, boxes=B * (G + S) * (36 + 4 + 1) * 2 + B * 60)
    res = dict(metric="centerpoint_augment_step", config="centerpoint_pp_nusc_train (min_points_in_gt 5, global_translate_std 0.2)", batch=B,
               points_per_sample=n, gt_per_sample=G, candidates_per_sample=S, points_per_candidate=per, steps=args.steps,
               kept_gt=int(keep.sum()), accepted=int(accept.sum()), rows_out=int(points()[1][-1]), boxes_out=out_count.cpu().tolist(), tbps=args.tbps)
    for key in timed:
        res[key + "_ms"] = round(med[key], 4)
        res[key + "_rounds_ms"] = [round(t, 4) for t in rounds[key]]
    for key, nb in nbytes.items():
        res[key + "_bytes"] = nb
        res[key + "_floor_us"] = round(nb / args.tbps / 1e6, 3)
        res[key + "_floor_share"] = round(nb / args.tbps / 1e9 / med[key], 5)
    res.update(ops_sum_ms=round(sum(med[k] for k in ("count", "select", "points", "boxes")), 4),
               augmentation_cost_ms=round(med["chain_augmented"] - med["chain_plain"], 4), equal_to_contract=equal)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
