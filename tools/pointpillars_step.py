"""Times the anchor-based KITTI PointPillars (configs/pointpillars/pointpillars_car_xyres16.py: RPN neck -> merged 1x1 heads ->
det_ops.PPHeadPost) on a seeded 496 x 432 x 64 pseudo-image with random weights and prints ONE JSON line (also written to --out):

  ms_per_step / samples_per_s   median of three event-timed rounds of `steps` forward passes (B = batch), after warm-up
  post_ms                       the head post-processing alone (PPHeadPost on the step's own head tensor: scores of every anchor, one
                                segmented top-k, decode of the selected anchors, NMS, gather), same timing
  composition_ms                the same result from the stand-alone operators, as the host code before PPHeadPost had to: sigmoid of
                                every class logit, det_ops.second_box_decode over ALL anchors, then per sample det_ops.pp_get_selected_data
                                (max / mask / top-k / gather / standup / NMS) -- rounds interleaved with post_ms in this process
  ratio                         composition_ms / post_ms (> 1: the fused chain is faster)
  nonempty_fraction             the fraction of pseudo-image cells that carry a pillar: a choice of this tool, not a KITTI statistic.
                                The clock of the post-processing depends on the data (how many anchors pass the score threshold)

Random weights: the detections are meaningless and the candidate lists are full (900 per sample), which is the expensive case of the
NMS.  python tools/pointpillars_step.py [--batch 4] [--steps 20] [--reps 20] [--nonempty 0.03] [--out profiles/...json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from minddet.models import Config, build_detector  # noqa: E402
from minddet_amd import det_ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nonempty", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointpillars_kitti_step_b4.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointpillars_step: needs the GPU (a time taken anywhere else says nothing)")
    dev = "cuda:0"
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", "pointpillars_car_xyres16.py"))
    model = build_detector(cfg.model, cfg.train_cfg, cfg.test_cfg).to(dev)
    g = torch.Generator().manual_seed(args.seed)
    B, (H, W) = args.batch, model.grid_hw
    x = torch.rand((B, H, W, 64), generator=g) * 1.5
    occ = torch.rand((B, H, W, 1), generator=g) < args.nonempty
    x = (x * occ).to(torch.bfloat16).to(dev)
    mask = torch.ones((B, model.anchors.shape[0]), dtype=torch.uint8, device=dev)

    for _ in range(3):
        (dets, count), aux = model.forward(x, anchors_mask=mask, return_aux=True)
    head, anchors = aux["head"], model.anchors
    A, K, off = model.num_anchors, model.num_class, model.head_offsets()
    N = anchors.shape[0]
    nms_cfg = {k: model.test_cfg[k] for k in ("nms_pre_max_size", "nms_post_max_size", "nms_score_threshold", "nms_iou_threshold")}
    maskb = mask.bool()

    def step():
        model.forward(x, anchors_mask=mask)

    def fused():
        model.post(head, anchors, mask)

    def composition():
        cls = det_ops.sigmoid_clip(head[..., off["cls"]:off["cls"] + A * K].float().reshape(B, N, K), 0.0, 1.0)
        boxes = det_ops.second_box_decode(head[..., off["box"]:off["box"] + 7 * A].float().reshape(B, N, 7), anchors)
        return [det_ops.pp_get_selected_data(cls[b], boxes[b], maskb[b], nms_cfg) for b in range(B)]

    fused(), composition(), step()
    torch.cuda.synchronize()
    same = all(int(n) == int(count[b]) for b, (_, _, _, n) in enumerate(composition()))
    ts, tf, tc = [], [], []
    for _ in range(3):
        ts.append(time_calls(step, args.steps))
        tf.append(time_calls(fused, args.reps))
        tc.append(time_calls(composition, args.reps))
    ms, f_ms, c_ms = statistics.median(ts), statistics.median(tf), statistics.median(tc)
    line = json.dumps(dict(
        metric="pointpillars_kitti_step", config="pointpillars_car_xyres16", batch=B, steps=args.steps, reps=args.reps,
        ms_per_step=round(ms, 3), samples_per_s=round(B / ms * 1e3, 1), rounds_ms=[round(t, 3) for t in ts],
        post_ms=round(f_ms, 4), post_rounds_ms=[round(t, 4) for t in tf], composition_ms=round(c_ms, 4),
        composition_rounds_ms=[round(t, 4) for t in tc], ratio=round(c_ms / f_ms, 2), counts_agree=same,
        post_share_of_step=round(f_ms / ms, 4), anchors=N, candidates=[int(c) for c in aux["topk_cnt"].cpu()],
        detections=[int(c) for c in count.cpu()], nonempty_fraction=round(float(occ.float().mean()), 4), weights="random"))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
