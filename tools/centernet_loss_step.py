"""Times the CenterNet training tail (det_ops.cn_assign_targets = md_cn_assign_targets, csrc/cntargets.hip; det_ops.cn_loss = md_cn_loss /
md_cn_loss_grad, csrc/cnloss.hip) at the shape of configs/centernet/centernet_r18_dcn_train.py -- B = 16, 80 classes on a 128 x 128 map
(an 88-channel head), max_objs 128 with about ten seeded objects per image, a seeded head tensor -- next to the same loss written with
torch device ops and autograd (below: fp32 on the widened head, no host read), and prints ONE JSON line (also written to --out).

  targets_ms / loss_ms / loss_grad_ms
                               median of three event-timed rounds of `steps` calls (outputs reused, as a training loop would); the
                               rounds of the five timed things are interleaved
  torch_forward_ms / torch_forward_backward_ms
                               the torch composition: the forward alone (under no_grad), and forward + autograd.grad to the head
  ratio_forward / ratio_forward_backward
                               torch time / operator time
  byte_floor                   per operator the bytes it has to move (targets: the heat map written once; loss: hm read twice -- the
                               count and the dense pass -- plus the bf16 head read; with grad plus the fp32 grad written), the time of
                               those bytes at --hbm-gbs and the measured time over it
  launches                     device kernels per call of each, counted by the profiler in a run of its own (null with the reason when
                               the profiler gives no kernel rows)
  kernels_us_per_call          the operators' kernels' device time per call, from the same profiled run
  total / torch_total, grad_max_abs_diff
                               the two results side by side (the torch composition computes in fp32: they agree to fp32 accuracy, not
                               to the last bit)
  equal_to_contract            the loss meets the conditions of tests/test_cn_loss_gpu.py against tests/cn_loss_contract.py, the
                               targets those of tests/test_cn_targets_gpu.py against tests/cn_targets_contract.py

python tools/centernet_loss_step.py [--steps 20] [--out profiles/centernet_loss_step_b16.json]
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
from minddet_amd import det_ops  # noqa: E402
from tests import cn_loss_contract as cl  # noqa: E402
from tests import cn_targets_contract as ct  # noqa: E402

KERNELS = ("cn_row_kernel", "cn_heat_kernel", "cn_loss_count_kernel", "cn_loss_dense_kernel", "cn_loss_finish_kernel")


class TorchLoss:
    """CenterNetLossCell.construct behind the network (centernet_det.py:206-237, utils.py:132-245) with torch device ops on the merged
    head tensor: the NHWC -> NCHW slice, sigmoid, clip, two logs, three pows, the selects and reductions of FocalLoss, and two
    gather + L1 RegLoss; fp32; nothing is read back by the host"""

    def __init__(self, loss, targets):
        self.l, self.t = loss, targets
        self.ind = targets["ind"].long()
        self.mask = targets["reg_mask"].to(torch.float32)

    def reg(self, feat, target):
        B, C = feat.shape[0], feat.shape[1]
        pred = feat.permute(0, 2, 3, 1).reshape(B, -1, C).gather(1, self.ind.unsqueeze(2).expand(-1, -1, C))
        m = self.mask.unsqueeze(2)
        return (pred * m - target * m).abs().sum() / (self.mask.sum() * 2 + 1e-4)

    def __call__(self, head):
        l, C = self.l, self.l.num_classes
        nchw = head.to(torch.float32).permute(0, 3, 1, 2)
        out = torch.clamp(torch.sigmoid(nchw[:, :C]), min=1e-4, max=1 - 1e-4)
        hm = self.t["hm"]
        pos_inds, neg_inds = (hm == 1.0).to(torch.float32), (hm < 1.0).to(torch.float32)
        pos = (torch.log(out) * torch.pow(1 - out, 2) * pos_inds).sum()
        neg = (torch.log(1 - out) * torch.pow(out, 2) * torch.pow(1 - hm, 4) * neg_inds).sum()
        num_pos = pos_inds.sum()
        num_pos = torch.where(num_pos == 0, torch.ones_like(num_pos), num_pos)
        total = l.hm_weight * (-(pos + neg) / num_pos) + l.wh_weight * self.reg(nchw[:, C:C + 2], self.t["wh"])
        if l.reg_offset and l.off_weight > 0:
            total = total + l.off_weight * self.reg(nchw[:, C + 2:C + 4], self.t["reg"])
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
    """-> (device kernels per call of each function, the operators' own kernels' device time in us per call, why either is missing),
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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--objects", type=float, default=10.0, help="expected objects per image")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the memory bandwidth the byte floor is priced at (MI355X peak: 8 TB/s)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "centernet_loss_step_b16.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("centernet_loss_step: needs the GPU (a time taken anywhere else says nothing)")
    dev = "cuda:0"
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centernet", "centernet_r18_dcn_train.py"))
    tgen = det_ops.CenterNetTargets.from_config(cfg)
    loss = det_ops.CenterNetLoss.from_config(cfg)
    B, G, C, (W, H) = args.batch, tgen.max_objs, tgen.num_classes, tgen.feature_map_size
    Cp = (C + 4 + 7) // 8 * 8
    rng = np.random.default_rng(args.seed)
    c = rng.uniform(0, W, (B, G, 2))
    s = np.exp(rng.uniform(np.log(2.0), np.log(90.0), (B, G, 2)))
    boxes_np = np.concatenate([c - s / 2, c + s / 2], -1).astype(np.float32)
    classes_np = np.where(rng.uniform(size=(B, G)) < args.objects / G, rng.integers(1, C + 1, (B, G)), 0).astype(np.int32)
    boxes, classes = torch.from_numpy(boxes_np).to(dev), torch.from_numpy(classes_np).to(dev)
    targets = tgen(boxes, classes)
    head = torch.from_numpy(rng.normal(-2.19, 2.0, (B, H, W, Cp)).astype(np.float32)).to(torch.bfloat16).to(dev)
    out_f, out_g = loss(head, targets), loss(head, targets, grad=True)
    tl = TorchLoss(loss, targets)
    leaf = head.clone().requires_grad_(True)

    fns = dict(targets=lambda: tgen(boxes, classes, out=targets), loss=lambda: loss(head, targets, out=out_f),
               loss_grad=lambda: loss(head, targets, grad=True, out=out_g), torch_forward=lambda: torch_no_grad(tl, head),
               torch_forward_backward=lambda: torch.autograd.grad(tl(leaf), leaf)[0])
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            rounds[k].append(time_calls(fn, args.steps))
    med = {k: statistics.median(v) for k, v in rounds.items()}

    got = {k: v.cpu().numpy() for k, v in fns["loss_grad"]().items()}
    tg = {k: v.cpu().numpy() for k, v in targets.items()}
    want_t = ct.assign(boxes_np, classes_np, num_classes=C, feature_map_size=(W, H), max_objs=G, min_overlap=tgen.min_overlap)
    nz = want_t["hm"] > 0
    apart = cl.ulps_apart(tg["hm"][nz], want_t["hm"][nz])
    targets_equal = all(np.array_equal(tg[k].view(np.uint8), want_t[k].view(np.uint8)) for k in ("ind", "reg_mask", "wh", "reg")) and \
        np.array_equal(tg["hm"] > 0, nz) and np.array_equal(tg["hm"] == 1, want_t["hm"] == 1) and int(apart.max()) <= 1 and \
        int((apart > 0).sum()) * 10000 <= int(nz.sum())
    want = cl.loss(head.to(torch.float32).cpu().numpy(), *(tg[k] for k in ct.KEYS), num_classes=C, off_hm=0, off_wh=C, off_reg=C + 2,
                   hm_weight=float(np.float32(loss.hm_weight)), wh_weight=float(np.float32(loss.wh_weight)),
                   off_weight=float(np.float32(loss.off_weight)))
    n, ndiff, worst, wrong_zero, nans = cl.compare_grad(got["grad"], want["grad"])
    equal = cl.compare_losses(got, want) <= 1 and worst <= 1 and ndiff * 10000 <= n and wrong_zero == 0 and nans == 0
    t_total, t_grad = float(torch_no_grad(tl, head)), fns["torch_forward_backward"]().to(torch.float32).cpu().numpy()

    hm_b, head_b, grad_b = 4 * B * C * H * W, 2 * B * H * W * Cp, 4 * B * H * W * Cp
    floor = {}
    for name, nbytes in (("targets", hm_b), ("loss", 2 * hm_b + head_b), ("loss_grad", 2 * hm_b + head_b + grad_b)):
        floor_ms = nbytes / (args.hbm_gbs * 1e9) * 1e3
        floor[name] = dict(bytes=nbytes, floor_ms=round(floor_ms, 4), measured_over_floor=round(med[name] / floor_ms, 2),
                           achieved_gbs=round(nbytes / (med[name] * 1e-3) / 1e9, 1))
    res = dict(
        metric="centernet_loss_step", config="centernet_r18_dcn_train", batch=B, steps=args.steps, head_shape=list(head.shape),
        hm_shape=list(targets["hm"].shape), max_objs=G, valid_slots=int(tg["reg_mask"].sum()), num_pos=float(got["num_pos"][0]),
        targets_ms=round(med["targets"], 4), loss_ms=round(med["loss"], 4), loss_grad_ms=round(med["loss_grad"], 4),
        torch_forward_ms=round(med["torch_forward"], 4), torch_forward_backward_ms=round(med["torch_forward_backward"], 4),
        rounds_ms={k: [round(t, 4) for t in v] for k, v in rounds.items()},
        ratio_forward=round(med["torch_forward"] / med["loss"], 2),
        ratio_forward_backward=round(med["torch_forward_backward"] / med["loss_grad"], 2),
        hbm_gbs=args.hbm_gbs, byte_floor=floor,
        launches=None, kernels_us_per_call=None, launches_missing="not measured yet",
        total=float(got["total"][0]), parts=[float(v) for v in got["parts"]], torch_total=t_total,
        grad_max_abs_diff=float(np.abs(t_grad - got["grad"]).max()), grad_max_abs=float(np.abs(got["grad"]).max()), grad_elements_owed=n,
        grad_differing_from_contract=ndiff, equal_to_contract=bool(equal), targets_equal_to_contract=bool(targets_equal))

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


def torch_no_grad(tl, head):
    with torch.no_grad():
        return tl(head)


if __name__ == "__main__":
    main()
