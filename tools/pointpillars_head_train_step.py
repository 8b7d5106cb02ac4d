"""Times the head training step of the KITTI PointPillars (optim.HeadTrainer: md_pp_loss_grad -> md_conv1x1_bwd_weight -> md_grad_sumsq ->
md_adam_step) at the Car shape of configs/pointpillars/pointpillars_car_xyres16_train.py -- B = 4, 248 x 216 x 384 neck features, the
24-channel merged head, targets from det_ops.assign_targets_batch on seeded ground truth -- next to the same weight gradient and update
written with torch device ops, and prints ONE JSON line (also written to --out).  The neck's features are seeded (bf16 N(0, 1) behind a
ReLU): the timed operators do not depend on their values, and the neck itself is timed only as part of train_step.

  wgrad_ms                     md_conv1x1_bwd_weight (both launches), median of three event-timed rounds of `steps` calls; the rounds of
                               everything timed are interleaved
  wgrad_kernels_us             its two kernels' device time per call, from a profiled run of its own (null with the reason otherwise)
  grad_sumsq_ms, adam_step_ms  the two optimizer operators on the head's flat range (32 x 384 + 32 elements)
  train_step_ms / forward_loss_ms
                               HeadTrainer.train_step from the pseudo-image against PointPillarsNet.loss(grad=True) alone
  torch_wgrad_ms, torch_adam_ms
                               the baseline: torch.einsum on the fp32-widened operands (x widened once outside the timed region would hide
                               its cost: it is widened inside, as a framework step does) and Adam written with torch ops, no host read
  wgrad_floor_us               x read once plus dy read once at 8 TB/s; wgrad_over_floor = wgrad time / floor
  wgrad_in_bound               the device result meets the Gaussian-data condition of tests/test_conv_bwd_gpu.py against the float64 contract

python tools/pointpillars_head_train_step.py [--steps 20] [--out profiles/pointpillars_head_train_step_b4.json]
Run each invocation under its own `timeout`."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from minddet.models import Config  # noqa: E402
from minddet_amd import det_ops  # noqa: E402
from minddet_amd.registry import build_detector  # noqa: E402
from tests import train_contract as tc  # noqa: E402
from tools.pointpillars_loss_step import ground_truth, time_calls  # noqa: E402

KERNELS = ("conv1x1_wgrad_kernel", "conv1x1_wgrad_sum_kernel", "grad_sumsq_kernel", "grad_sumsq_finish_kernel", "adam_step_kernel")


def kernel_times(fns, reps):
    """-> ({function: {kernel: us per call}}, why it is missing)"""
    try:
        from torch.profiler import ProfilerActivity, profile

        out = {}
        for name, fn in fns.items():
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
            for ev in prof.key_averages():
                for kn in KERNELS:
                    if kn + "<" in ev.key or kn + "(" in ev.key or ev.key.endswith(kn):
                        t = float(getattr(ev, "device_time_total", 0) or getattr(ev, "cuda_time_total", 0))
                        out.setdefault(name, {})[kn] = round(out.get(name, {}).get(kn, 0.0) + t / reps, 3)
        return (out, None) if out else (None, "the profiler reported none of the operators' kernels")
    except Exception as e:  # the measurement is optional; say why it is missing
        return None, f"{type(e).__name__}: {e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointpillars_head_train_step_b4.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointpillars_head_train_step: needs the GPU (a time taken anywhere else says nothing)")
    dev = "cuda:0"
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", "pointpillars_car_xyres16_train.py"))
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).to(dev)
    net, B = model.inner, args.batch
    H, W = net.feature_hw
    rng = np.random.default_rng(args.seed)
    boxes = [torch.from_numpy(ground_truth(rng, cfg, 20)).to(dev) for _ in range(B)]
    asg = cfg.train_cfg["assigner"]
    labels, reg, _, _ = det_ops.assign_targets_batch(net.anchors, boxes, None, asg["matched_threshold"], asg["unmatched_threshold"])
    example = dict(labels=labels, reg_targets=reg)
    g = torch.Generator().manual_seed(args.seed)
    canvas = (torch.randn((B, net.grid_hw[0], net.grid_hw[1], 64), generator=g) * (torch.rand((B, net.grid_hw[0], net.grid_hw[1], 1), generator=g) < 0.1))
    canvas = canvas.to(torch.bfloat16).to(dev)
    tr = net.head_trainer()
    pc, opt = net.bbox_head._merged, tr.opt
    rows, kpad = pc.w.shape
    feat = torch.relu(torch.randn((B, H, W, pc.cin), generator=g)).to(torch.bfloat16).to(dev)
    out = net.loss_op()(net.bbox_head(feat), labels, reg, net.anchors, grad=True)
    dy = out["grad"]
    dw, db = opt.view("w", "grad"), opt.view("b", "grad")
    sumsq = torch.zeros((1,), dtype=torch.float64, device=dev)
    state = opt.state()

    # the torch baseline: fp32-widened operands, einsum, Adam with torch ops (the reference's order), nothing read back
    tp, tm, tv = opt.param.clone(), torch.zeros_like(opt.param), torch.zeros_like(opt.param)
    tg = torch.zeros_like(opt.param)

    def torch_wgrad():
        x32 = feat.to(torch.float32).reshape(-1, pc.cin)
        d = dy.reshape(-1, dy.shape[-1])
        tg[:rows * kpad].view(rows, kpad)[:d.shape[1], :pc.cin] = torch.einsum("po,pi->oi", d, x32)
        tg[rows * kpad:][:d.shape[1]] = d.sum(0)

    def torch_adam(lr=2e-4, b1=0.9, b2=0.999, eps=1e-8, wd=1e-4, b1p=0.9, b2p=0.999):
        grad = tg + wd * tp
        tm.mul_(b1).add_(grad, alpha=1 - b1)
        tv.mul_(b2).addcmul_(grad, grad, value=1 - b2)
        tp.sub_(lr * (1 - b2p) ** 0.5 / (1 - b1p) * tm / (tv.sqrt() + eps))

    fns = dict(
        wgrad=lambda: det_ops.conv1x1_bwd_weight(feat, dy, pc, out=(dw, db)),
        grad_sumsq=lambda: det_ops.grad_sumsq(opt.grad, out=sumsq),
        adam_step=lambda: opt.step(2e-4, 0.9),
        train_step=lambda: tr.train_step(canvas, example, 2e-4, 0.9),
        forward_loss=lambda: net.loss(canvas, example, grad=True),
        torch_wgrad=torch_wgrad, torch_adam=torch_adam)
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            rounds[k].append(time_calls(fn, args.steps))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    opt.load_state(state)

    fns["wgrad"]()
    torch.cuda.synchronize()
    x_np, dy_np = feat.float().cpu().numpy(), dy.cpu().numpy()
    P = B * H * W
    want = tc.wgrad(x_np, dy_np, pc.cin, pc.cout, rows=rows, kpad=kpad)
    err = np.abs(dw.cpu().numpy().astype(np.float64) - want["dw"])
    bound = tc.wgrad_bound(P, want["absdw"])
    live = want["absdw"] > 0
    floor_us = (feat.numel() * 2 + dy.numel() * 4) / 8e12 * 1e6
    res = dict(
        metric="pointpillars_head_train_step", config="pointpillars_car_xyres16_train", batch=B, steps=args.steps,
        features_shape=list(feat.shape), head_grad_shape=list(dy.shape), pack_shape=[rows, kpad], flat_range=int(opt.n),
        wgrad_ms=round(med["wgrad"], 4), grad_sumsq_ms=round(med["grad_sumsq"], 4), adam_step_ms=round(med["adam_step"], 4),
        train_step_ms=round(med["train_step"], 4), forward_loss_ms=round(med["forward_loss"], 4),
        torch_wgrad_ms=round(med["torch_wgrad"], 4), torch_adam_ms=round(med["torch_adam"], 4),
        rounds_ms={k: [round(t, 4) for t in v] for k, v in rounds.items()},
        wgrad_floor_us=round(floor_us, 2), wgrad_over_floor=round(med["wgrad"] * 1e3 / floor_us, 2),
        ratio_torch_wgrad=round(med["torch_wgrad"] / med["wgrad"], 2), chain_length=tc.chain_length(P),
        wgrad_worst_error_over_bound=float((err[live] / bound[live]).max()), wgrad_in_bound=bool((err <= bound).all()),
        wgrad_kernels_us=None, kernels_missing="not measured yet")

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(res) + "\n")

    write()                                           # the times are on disk before the profiled run starts
    kernels, why = kernel_times({k: fns[k] for k in ("wgrad", "grad_sumsq", "adam_step")}, 3)
    res.update(wgrad_kernels_us=kernels, kernels_missing=why)
    write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
