"""Times the KITTI PointPillars training loss (det_ops.pp_loss = md_pp_loss / md_pp_loss_grad, csrc/pploss.hip) at the Car shape of
configs/pointpillars/pointpillars_car_xyres16_train.py -- B = 4, 248 x 216 cells, 2 anchors per cell (107 136 per sample), targets from
det_ops.assign_targets_batch on seeded ground truth, a seeded head tensor -- next to the same loss written with torch device ops and
autograd (below: fp32 on the widened head, no host read), and prints ONE JSON line (also written to --out).

  loss_ms / loss_grad_ms       median of three event-timed rounds of `steps` calls of md_pp_loss / md_pp_loss_grad (outputs reused, as a
                               training loop would); the rounds of the four timed things are interleaved
  torch_forward_ms / torch_forward_backward_ms
                               the torch composition: the forward alone (under no_grad), and forward + autograd.grad to the head
  ratio_forward / ratio_forward_backward
                               torch time / operator time
  launches                     device kernels per call of each, counted by the profiler in a run of its own (null with the reason when
                               the profiler gives no kernel rows); the operator's three are also what csrc/pploss.hip states
  kernels_us_per_call          the three kernels' device time per call of md_pp_loss and of md_pp_loss_grad, from the same profiled run
  total / torch_total, grad_max_abs_diff
                               the two results side by side (the torch composition computes in fp32: they agree to fp32 accuracy, not
                               to the last bit)
  equal_to_contract            the operator's result meets the conditions of tests/test_pp_loss_gpu.py against tests/pp_loss_contract.py

python tools/pointpillars_loss_step.py [--steps 20] [--out profiles/pointpillars_loss_step_b4.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from minddet.models import Config  # noqa: E402
from minddet_amd import det_ops  # noqa: E402
from tests import pp_loss_contract as pl  # noqa: E402

KERNELS = ("pp_loss_count_kernel", "pp_loss_dense_kernel", "pp_loss_finish_kernel")


def ground_truth(rng, cfg, count):
    """`count` Car-sized boxes (x, y, z, w, l, h, r) inside the config's range"""
    g = cfg.model["anchor_generators"][0]
    x0, y0, _, x1, y1, _ = cfg.model["voxel_generator"]["point_cloud_range"]
    gt = np.zeros((count, 7), np.float32)
    gt[:, 0], gt[:, 1] = rng.uniform(x0 + 2, x1 - 2, count), rng.uniform(y0 + 2, y1 - 2, count)
    gt[:, 2] = g["offsets"][2] + rng.uniform(-0.2, 0.2, count)
    gt[:, 3:6] = np.array(g["sizes"]) * rng.uniform(0.9, 1.1, (count, 3))
    gt[:, 6] = rng.choice([0.0, 1.57, -1.57, 3.1], count) + rng.uniform(-0.2, 0.2, count)
    return gt


class TorchLoss:
    """PointPillarsWithLossCell.construct behind the network (pointpillars.py:817-872, losses.py:40-191) with torch device ops on the
    merged head tensor: a one-hot, sigmoid / log1p / exp / pow over every anchor and class, sin / cos over every anchor, a softmax
    cross-entropy and the reductions; fp32; nothing is read back by the host"""

    def __init__(self, loss, labels, reg_targets, anchors):
        self.l, self.A, self.K = loss, loss.num_anchors, loss.num_classes
        dev = labels.device
        pos, neg = labels > 0, labels == 0
        nb = pos.sum(1, keepdim=True).to(torch.float32).clamp(min=1.0)
        self.cls_w = ((pos * loss.pos_cls_weight + neg * loss.neg_cls_weight) / nb).unsqueeze(2)
        self.reg_w = (pos / nb).unsqueeze(2)
        self.dir_w = pos / nb
        self.one_hot = F.one_hot((labels * (labels >= 0)).long(), self.K + 1)[..., 1:].to(torch.float32)
        self.pos, self.neg = pos, neg
        self.tgt = reg_targets
        self.sin_t, self.cos_t = torch.sin(reg_targets[..., 6:]), torch.cos(reg_targets[..., 6:])
        self.dir_t = ((reg_targets[..., 6] + anchors[None, :, 6]) > 0).long()
        self.cw = torch.tensor(loss.code_weights, dtype=torch.float32, device=dev).view(1, 1, -1)

    def __call__(self, head):
        l, A, K = self.l, self.A, self.K
        B = head.shape[0]
        off = l.head_offsets
        flat = head.to(torch.float32)
        x = flat[..., off["cls"]:off["cls"] + A * K].reshape(B, -1, K)
        box = flat[..., off["box"]:off["box"] + A * 7].reshape(B, -1, 7)
        z = self.one_hot
        ce = torch.clamp(x, min=0) - x * z + torch.log1p(torch.exp(-torch.abs(x)))
        p = torch.sigmoid(x)
        p_t = z * p + (1 - z) * (1 - p)
        mod = torch.pow(1.0 - p_t, l.gamma) if l.gamma else 1.0
        alpha_w = z * l.alpha + (1 - z) * (1 - l.alpha) if l.alpha is not None else 1.0
        cls = (mod * alpha_w * ce * self.cls_w).sum() / B * l.cls_weight
        pred = torch.cat([box[..., :6], torch.sin(box[..., 6:]) * self.cos_t], -1)
        tgt = torch.cat([self.tgt[..., :6], torch.cos(box[..., 6:]) * self.sin_t], -1)
        ad = torch.abs(self.cw * (pred - tgt))
        lt = (ad <= 1 / l.sigma ** 2).to(torch.float32)
        loc = ((lt * 0.5 * torch.pow(ad * l.sigma, 2) + (ad - 0.5 / l.sigma ** 2) * (1.0 - lt)) * self.reg_w).sum() / B * l.loc_weight
        total = loc + cls
        if off.get("dir_cls") is not None:
            d = flat[..., off["dir_cls"]:off["dir_cls"] + A * 2].reshape(-1, 2)
            dir_loss = (F.cross_entropy(d, self.dir_t.reshape(-1), reduction="none").view(B, -1) * self.dir_w).sum() / B
            total = total + dir_loss * l.dir_weight
        return total


def time_calls(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def count_launches(fns, reps):
    """-> (device kernels per call of each function, the operator's own kernels' device time in us per call, why either is missing),
    from one profiled run of `reps` calls each"""
    try:
        from torch.profiler import ProfilerActivity, profile

        out, kernels = {}, {}
        for name, fn in fns.items():
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
            n = sum(int(ev.count) for ev in prof.key_averages()
                    if float(getattr(ev, "device_time_total", 0) or getattr(ev, "cuda_time_total", 0)) > 0 and "memcpy" not in ev.key.lower()
                    and "memset" not in ev.key.lower())
            if n == 0:
                return None, None, f"the profiler reported no device kernels for {name}"
            out[name] = round(n / reps, 2)
            for ev in prof.key_averages():
                for kn in KERNELS:
                    if kn in ev.key:
                        t = float(getattr(ev, "device_time_total", 0) or getattr(ev, "cuda_time_total", 0))
                        kernels.setdefault(name, {})[kn] = round(kernels.get(name, {}).get(kn, 0.0) + t / reps, 3)
        return out, kernels, None
    except Exception as e:  # the measurement is optional; say why it is missing
        return None, None, f"{type(e).__name__}: {e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointpillars_loss_step_b4.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointpillars_loss_step: needs the GPU (a time taken anywhere else says nothing)")
    dev = "cuda:0"
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", "pointpillars_car_xyres16_train.py"))
    H, W = cfg.data["feature_map_hw"]
    gens = [det_ops.AnchorGeneratorStride(sizes=g["sizes"], anchor_strides=g["strides"], anchor_offsets=g["offsets"], rotations=g["rotations"],
                                          anchor_range=cfg.model["voxel_generator"]["point_cloud_range"]) for g in cfg.model["anchor_generators"]]
    A, K, B = sum(g.num_anchors_per_localization for g in gens), cfg.model["num_class"], args.batch
    anchors = det_ops.generate_anchors(gens, (1, H, W), device=dev)["anchors"].reshape(-1, 7)
    rng = np.random.default_rng(args.seed)
    boxes = [torch.from_numpy(ground_truth(rng, cfg, 20)).to(dev) for _ in range(B)]
    asg = cfg.train_cfg["assigner"]
    labels, reg, _, _ = det_ops.assign_targets_batch(anchors, boxes, None, asg["matched_threshold"], asg["unmatched_threshold"])
    offs = dict(cls=0, box=A * K, dir_cls=A * K + A * 7)          # PPAnchorHead.head_offsets() of this config
    C = (A * (K + 9) + 7) // 8 * 8
    loss = det_ops.PointPillarsLoss(offs, A, K, cfg.train_cfg["loss"], cfg.train_cfg["direction_loss_weight"], cfg.train_cfg["pos_class_weight"],
                                    cfg.train_cfg["neg_class_weight"])
    h = rng.normal(0, 1.5, (B, H, W, C)).astype(np.float32)
    h[..., :A * K] = np.clip(rng.normal(-2.0, 3.0, (B, H, W, A * K)), -12, 12)
    head = torch.from_numpy(h).to(torch.bfloat16).to(dev)
    out_f, out_g = loss(head, labels, reg, anchors), loss(head, labels, reg, anchors, grad=True)
    tl = TorchLoss(loss, labels, reg, anchors)
    leaf = head.clone().requires_grad_(True)

    def op_forward():
        return loss(head, labels, reg, anchors, out=out_f)

    def op_grad():
        return loss(head, labels, reg, anchors, grad=True, out=out_g)

    def torch_forward():
        with torch.no_grad():
            return tl(head)

    def torch_backward():
        return torch.autograd.grad(tl(leaf), leaf)[0]

    fns = dict(loss=op_forward, loss_grad=op_grad, torch_forward=torch_forward, torch_forward_backward=torch_backward)
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            rounds[k].append(time_calls(fn, args.steps))
    med = {k: statistics.median(v) for k, v in rounds.items()}

    got = {k: v.cpu().numpy() for k, v in op_grad().items()}
    want = pl.loss(head.to(torch.float32).cpu().numpy(), labels.cpu().numpy(), reg.cpu().numpy(), anchors.cpu().numpy(), off_cls=offs["cls"],
                   off_box=offs["box"], off_dir=offs["dir_cls"], num_anchors=A, num_classes=K, alpha=loss.alpha, gamma=loss.gamma,
                   sigma=loss.sigma, code_weights=loss.code_weights, cls_weight=loss.cls_weight, loc_weight=loss.loc_weight,
                   dir_weight=loss.dir_weight, pos_cls_weight=loss.pos_cls_weight, neg_cls_weight=loss.neg_cls_weight)
    n, ndiff, worst, wrong_zero, nans = pl.compare_grad(got["grad"], want)
    equal = pl.compare_losses(got, want) <= 1 and worst <= 1 and ndiff * 10000 <= n and wrong_zero == 0 and nans == 0
    t_total, t_grad = float(torch_forward()), torch_backward().to(torch.float32).cpu().numpy()
    res = dict(
        metric="pointpillars_loss_step", config="pointpillars_car_xyres16_train", batch=B, anchors_per_sample=int(anchors.shape[0]),
        steps=args.steps, head_shape=list(head.shape), num_pos=[int(v) for v in got["num_pos"]],
        ignored=[int(v) for v in (labels < 0).sum(1).tolist()],
        loss_ms=round(med["loss"], 4), loss_grad_ms=round(med["loss_grad"], 4), torch_forward_ms=round(med["torch_forward"], 4),
        torch_forward_backward_ms=round(med["torch_forward_backward"], 4),
        rounds_ms={k: [round(t, 4) for t in v] for k, v in rounds.items()},
        ratio_forward=round(med["torch_forward"] / med["loss"], 2),
        ratio_forward_backward=round(med["torch_forward_backward"] / med["loss_grad"], 2),
        launches=None, kernels_us_per_call=None, launches_missing="not measured yet",
        total=float(got["total"][0]), parts=[float(v) for v in got["parts"]], torch_total=t_total,
        grad_max_abs_diff=float(np.abs(t_grad - got["grad"]).max()), grad_max_abs=float(np.abs(got["grad"]).max()), grad_elements_owed=n,
        grad_differing_from_contract=ndiff, equal_to_contract=bool(equal))

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(res) + "\n")

    write()                                           # the times are on disk before the profiled run starts
    launches, kernels_us, why = count_launches(fns, 3)
    res.update(launches=launches, kernels_us_per_call=kernels_us, launches_missing=why)
    write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
