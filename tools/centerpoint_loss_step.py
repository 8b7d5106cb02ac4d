"""Times the CenterPoint training loss (det_ops.cp_loss = md_cp_loss / md_cp_loss_grad, csrc/cploss.hip) at the nuScenes shape of
configs/centerpoint/centerpoint_pp_nusc_train.py -- B = 4, six tasks, 128 x 128 maps, max_objs 500, targets from
det_ops.cp_assign_targets on 500 seeded objects per sample, the head tensor from graphs.CenterHead on random input -- next to the same
loss written with torch device ops and autograd (below: fp32 on the widened head, no host read), and prints ONE JSON line (also
written to --out).

  loss_ms / loss_grad_ms       median of three event-timed rounds of `steps` calls of md_cp_loss / md_cp_loss_grad (outputs reused, as a
                               training loop would); the rounds of the four timed things are interleaved
  torch_forward_ms / torch_forward_backward_ms
                               the torch composition: the forward alone (under no_grad), and forward + autograd.grad to the head
  ratio_forward / ratio_forward_backward
                               torch time / operator time
  launches                     device kernels per call of each, counted by the profiler in a run of its own (null with the reason when
                               the profiler gives no kernel rows); the operator's three are also what csrc/cploss.hip states
  kernels_us_per_call          the three kernels' device time per call of md_cp_loss and of md_cp_loss_grad, from the same profiled run
  total / torch_total, grad_max_abs_diff
                               the two results side by side (the torch composition computes in fp32: they agree to fp32 accuracy, not
                               to the last bit)
  equal_to_contract            the operator's result meets the conditions of tests/test_cp_loss_gpu.py against tests/cp_loss_contract.py

python tools/centerpoint_loss_step.py [--steps 20] [--out profiles/centerpoint_loss_step_b4.json]
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
from minddet.models import Config  # noqa: E402
from minddet_amd import det_ops, graphs  # noqa: E402
from tests import cp_loss_contract as cl  # noqa: E402

KEYS = ("hm", "anno_box", "ind", "mask", "cat")


def inputs(B, G, seed):
    rng = np.random.default_rng(seed)
    b = np.zeros((B, G, 9), np.float32)
    b[..., 0:2] = rng.uniform(-51.0, 51.0, (B, G, 2))
    b[..., 2] = rng.uniform(-4, 2, (B, G))
    b[..., 3:5] = np.exp(rng.uniform(np.log(0.3), np.log(14.0), (B, G, 2)))
    b[..., 5] = rng.uniform(0.5, 4.0, (B, G))
    b[..., 6:8] = rng.normal(0, 4, (B, G, 2))
    b[..., 8] = rng.uniform(-3.2, 3.2, (B, G))
    return b, rng.integers(1, 11, (B, G)).astype(np.int32)


class TorchLoss:
    """CenterHead.loss (center_head.py:208-271, centernet_loss.py:22-82) with torch device ops on the merged head tensor: per task a
    channel slice, sigmoid, clamp, pows, a log, gathers and reductions; fp32; nothing is read back by the host"""

    def __init__(self, task_offsets, num_classes, weight, code_weights, targets):
        self.weight, self.tasks = float(weight), []
        for t, (off, nc) in enumerate(zip(task_offsets, num_classes)):
            chans, tcols = cl.columns(off)
            dev = targets["hm"].device
            B, M = targets["ind"].shape[0], targets["ind"].shape[2]
            mask = targets["mask"][:, t].to(torch.float32).unsqueeze(2)
            self.tasks.append(dict(
                hm0=off["hm"], nc=nc, chans=torch.as_tensor(chans, device=dev), mask=mask, num=mask.sum(),
                g4=(1 - targets["hm"][:, t, :nc].reshape(B, nc, -1).transpose(1, 2)).pow(4),
                ind=targets["ind"][:, t].long().unsqueeze(2), cat=targets["cat"][:, t].long().unsqueeze(2),
                box=targets["anno_box"][:, t][..., torch.as_tensor(tcols, device=dev)] * mask,
                cw=torch.tensor([float(v) for v in code_weights][:len(chans)], dtype=torch.float32, device=dev)))

    def __call__(self, head):
        B, H, W, Cp = head.shape
        flat = head.to(torch.float32).view(B, H * W, Cp)
        total = 0
        for k in self.tasks:
            p = torch.clamp(torch.sigmoid(flat[..., k["hm0"]:k["hm0"] + k["nc"]]), min=1e-4, max=1 - 1e-4)
            neg = (torch.log(1 - p) * p.pow(2) * k["g4"]).sum()
            pp = p.gather(1, k["ind"].expand(-1, -1, k["nc"])).gather(2, k["cat"])
            pos = (torch.log(pp) * (1 - pp).pow(2) * k["mask"]).sum()
            hm_loss = torch.where(k["num"] == 0, -neg, -(pos + neg) / k["num"].clamp(min=1))
            pred = flat.gather(1, k["ind"].expand(-1, -1, Cp))[..., k["chans"]]
            box_loss = ((pred * k["mask"] - k["box"]).abs() / (k["num"] + 1e-4)).sum((0, 1))
            total = total + hm_loss + self.weight * (box_loss * k["cw"]).sum()
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
                for kn in ("cp_loss_slot_kernel", "cp_loss_dense_kernel", "cp_loss_finish_kernel"):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "centerpoint_loss_step_b4.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("centerpoint_loss_step: needs the GPU (a time taken anywhere else says nothing)")
    dev = "cuda:0"
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc_train.py"))
    tgen = det_ops.CenterPointTargets.from_config(cfg)
    B, G = args.batch, tgen.max_objs
    boxes, classes = inputs(B, G, args.seed)
    targets = tgen(torch.from_numpy(boxes).to(dev), torch.from_numpy(classes).to(dev))
    head_mod = graphs.CenterHead(**{k: v for k, v in cfg.model["bbox_head"].items() if k != "type"}, **cfg.train_cfg["loss"]).to(dev)
    W, H = tgen.feature_map_size
    rng = np.random.default_rng(args.seed + 1)
    x = torch.from_numpy(rng.normal(0, 1, (B, H, W, head_mod.in_channels)).astype(np.float32)).to(torch.bfloat16).to(dev)
    head, _ = head_mod(x)
    head = torch.nan_to_num(head, nan=0.0)                 # the pad channels the head conv does not write: the torch gather reads them
    loss = det_ops.CenterPointLoss.from_config(cfg, head_mod)
    out_f, out_g = loss(head, targets), loss(head, targets, grad=True)
    tl = TorchLoss(head_mod.task_offsets(), head_mod.num_classes, loss.weight, loss.code_weights, targets)
    leaf = head.clone().requires_grad_(True)

    def op_forward():
        return loss(head, targets, out=out_f)

    def op_grad():
        return loss(head, targets, grad=True, out=out_g)

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
    tg = {k: targets[k].cpu().numpy() for k in KEYS}
    want = cl.loss(head.to(torch.float32).cpu().numpy(), *(tg[k] for k in KEYS), task_offsets=head_mod.task_offsets(),
                   num_classes=head_mod.num_classes, weight=float(np.float32(loss.weight)),
                   code_weights=[float(np.float32(v)) for v in loss.code_weights])
    nnz, ndiff, worst, wrong_zero, nans = cl.compare_grad(got["grad"], want["grad"])
    equal = cl.compare_losses(got, want) <= 1 and worst <= 1 and ndiff * 10000 <= nnz and wrong_zero == 0 and nans == 0
    t_total, t_grad = float(torch_forward()), torch_backward().to(torch.float32).cpu().numpy()
    res = dict(
        metric="centerpoint_loss_step", config="centerpoint_pp_nusc_train", batch=B, objects_per_sample=G, steps=args.steps,
        head_shape=list(head.shape), num_pos=[int(v) for v in got["num_pos"]],
        loss_ms=round(med["loss"], 4), loss_grad_ms=round(med["loss_grad"], 4), torch_forward_ms=round(med["torch_forward"], 4),
        torch_forward_backward_ms=round(med["torch_forward_backward"], 4),
        rounds_ms={k: [round(t, 4) for t in v] for k, v in rounds.items()},
        ratio_forward=round(med["torch_forward"] / med["loss"], 2),
        ratio_forward_backward=round(med["torch_forward_backward"] / med["loss_grad"], 2),
        launches=None, kernels_us_per_call=None, launches_missing="not measured yet",
        total=float(got["total"][0]), torch_total=t_total, grad_max_abs_diff=float(np.abs(t_grad - got["grad"]).max()),
        grad_max_abs=float(np.abs(got["grad"]).max()), grad_nonzero=nnz, grad_differing_from_contract=ndiff,
        equal_to_contract=bool(equal))

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
