"""Times the head training step of CenterPoint (optim.CenterPointHeadTrainer: md_cp_loss_grad -> md_conv2d_grouped_bwd_weight ->
md_conv2d_grouped_bwd_data (through the first convs' ReLU) -> md_conv_bwd_weight (the merged first convs, in chunks of 256 output
channels) -> md_grad_sumsq -> md_adam_step) at the nuScenes shape -- configs/centerpoint/centerpoint_pp_nusc.py with the train settings of
centerpoint_pp_nusc_train.py, B = 4, a 128 x 128 head, six tasks = 36 SepHead branches -- on a seeded pseudo-image and seeded boxes, next to
the same gradients from torch on the fp32-widened operands, and prints ONE JSON line (also written to --out).

  gwgrad_ms, gdgrad_ms             md_conv2d_grouped_bwd_weight, md_conv2d_grouped_bwd_data: median of three event-timed rounds of `steps`
                                   calls; the rounds of everything timed are interleaved
  wgrad1_ms                        the merged first convs' weight gradient: nine md_conv_bwd_weight calls of 256 output channels
  adam_ms                          md_grad_sumsq + md_adam_step on the one flat range
  train_step_ms / forward_loss_ms  PointPillars.train_step from the pseudo-image against PointPillars.loss(grad=True) alone
  torch_*_ms                       torch.nn.grad.conv2d_weight / conv2d_input with groups = 36 (every group widened to three outputs) and
                                   the ReLU mask, on the operands widened to fp32 inside the timed region, as a framework step does; null
                                   with the reason where torch could not run it
  *_byte_floor_us                  the operator's operands and results once at 8 TB/s
  *_product_floor_us               the operator's multiply-adds at the fp32 MFMA rate, 157 TFLOP/s (gwgrad: the 16-row tiles it runs)

python tools/centerpoint_head_train_step.py [--steps 20] [--out profiles/centerpoint_head_train_step_b4.json]
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
from tools.pointpillars_loss_step import time_calls  # noqa: E402

HBM, MFMA_F32 = 8e12, 157e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch baselines")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "centerpoint_head_train_step_b4.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("centerpoint_head_train_step: needs the GPU (a time taken anywhere else says nothing)")
    dev = "cuda:0"
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc.py"))
    tcfg = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc_train.py"))
    net = build_detector(dict(cfg.model), train_cfg=dict(tcfg.train_cfg), test_cfg=cfg.test_cfg).to(dev)
    B = args.batch
    rng = np.random.default_rng(args.seed)
    tgen = det_ops.CenterPointTargets.from_config(tcfg)
    G = tgen.max_objs
    b = np.zeros((B, G, 9), np.float32)
    b[..., 0:2] = rng.uniform(-50, 50, (B, G, 2))
    b[..., 2] = rng.uniform(-4, 2, (B, G))
    b[..., 3:5] = np.exp(rng.uniform(np.log(0.3), np.log(14.0), (B, G, 2)))
    b[..., 5] = rng.uniform(0.5, 4.0, (B, G))
    b[..., 6:8] = rng.normal(0, 4, (B, G, 2))
    b[..., 8] = rng.uniform(-3.0, 3.0, (B, G))
    ex = tgen(torch.from_numpy(b).to(dev), torch.from_numpy(rng.integers(1, 11, (B, G)).astype(np.int32)).to(dev))
    occupied = torch.from_numpy(rng.uniform(size=(B, 512, 512, 1)) < 0.1).to(dev)
    pi = (torch.randn((B, 512, 512, 64), device=dev, generator=torch.Generator(device=dev).manual_seed(args.seed)).clamp_(min=0) * occupied).to(torch.bfloat16)
    tr = net.head_trainer()
    opt, head = tr.opt, net.bbox_head
    pc1, pk2 = head._first, head._second
    state = opt.state()
    lr, beta1 = 1e-3, 0.95
    first = net.train_step(pi, ex, lr, beta1)
    feat, sh, mid, g = first["neck"], first["shared"], first["mid"], first["grad"]
    dmid = torch.empty_like(first["dmid"])
    del first
    N, H, W, _ = mid.shape
    P, Gr, CM = N * H * W, pk2.groups, max(pk2.couts)
    gw, gb = opt.view("w1", "grad"), opt.view("b1", "grad")

    def wgrad1():
        for r0 in range(0, pc1.cout, tr.FIRST_CHUNK):
            n = min(tr.FIRST_CHUNK, pc1.cout - r0)
            r1 = gw.shape[0] if r0 + n == pc1.cout else r0 + n
            det_ops.conv_bwd_weight(sh, dmid, pc1, dy_c_off=r0, cout=n, out=(gw[r0:r1], gb[r0:r1]))

    # torch: the grouped conv with every group widened to CM outputs (rows past cout zero)
    w32 = torch.zeros((Gr * CM, 64, 3, 3), device=dev)
    sel = []
    for i in range(Gr):
        r0, c = pk2.w_rows[i], pk2.couts[i]
        w32[i * CM:i * CM + c] = pk2.w[r0:r0 + c].float().reshape(c, 3, 3, 64).permute(0, 3, 1, 2)
        sel += [pk2.y_offs[i] + min(o, c - 1) for o in range(CM)]
    sel = torch.tensor(sel, device=dev)
    live = torch.tensor([o < pk2.couts[i] for i in range(Gr) for o in range(CM)], device=dev).view(1, -1, 1, 1)

    def wide_dy():
        return g.permute(0, 3, 1, 2)[:, sel] * live

    def torch_gwgrad():
        return torch.nn.grad.conv2d_weight(mid.float().permute(0, 3, 1, 2), tuple(w32.shape), wide_dy(), padding=1, groups=Gr), g.sum((0, 1, 2))

    def torch_gdgrad():
        d = torch.nn.grad.conv2d_input((N, 64 * Gr, H, W), w32, wide_dy(), padding=1, groups=Gr)
        return d * (mid.permute(0, 3, 1, 2) > 0)

    def torch_wgrad1():
        return torch.nn.grad.conv2d_weight(sh.float().permute(0, 3, 1, 2), (pc1.cout, 64, 3, 3), dmid.permute(0, 3, 1, 2), padding=1), dmid.sum((0, 1, 2))

    fns = dict(
        gwgrad=lambda: det_ops.conv2d_grouped_bwd_weight(mid, g, pk2, out=(opt.view("w2", "grad"), opt.view("b2", "grad"))),
        gdgrad=lambda: det_ops.conv2d_grouped_bwd_data(g, pk2, act=mid, out=dmid),
        wgrad1=wgrad1, adam=lambda: opt.step(lr, beta1),
        train_step=lambda: net.train_step(pi, ex, lr, beta1), forward_loss=lambda: net.loss(pi, ex, grad=True))
    fns["gdgrad"]()
    missing = {}
    if not args.no_torch:
        for name, fn in (("torch_gwgrad", torch_gwgrad), ("torch_gdgrad", torch_gdgrad), ("torch_wgrad1", torch_wgrad1)):
            try:
                fn()
                torch.cuda.synchronize()
                fns[name] = fn
            except Exception as e:  # the baseline is optional; say why it is missing
                missing[name] = f"{type(e).__name__}: {e}"
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            rounds[k].append(time_calls(fn, args.steps))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    opt.load_state(state)

    def floors(name, nbytes, macs):
        return {f"{name}_byte_floor_us": round(nbytes / HBM * 1e6, 2), f"{name}_product_floor_us": round(2 * macs / MFMA_F32 * 1e6, 2),
                f"{name}_over_byte_floor": round(med[name] * 1e3 / (nbytes / HBM * 1e6), 2),
                f"{name}_over_product_floor": round(med[name] * 1e3 / (2 * macs / MFMA_F32 * 1e6), 2)}

    ratio = lambda a, b: round(med[a] / med[b], 2) if a in med else None
    res = dict(
        metric="centerpoint_head_train_step", config="centerpoint_pp_nusc + centerpoint_pp_nusc_train", batch=B, steps=args.steps,
        shared_shape=list(sh.shape), mid_shape=list(mid.shape), head_grad_shape=list(g.shape), first_pack_shape=list(pc1.w.shape),
        second_pack_shape=list(pk2.w.shape), groups=Gr, flat_parameters=opt.n,
        **{k + "_ms": round(v, 4) for k, v in med.items()}, rounds_ms={k: [round(t, 4) for t in v] for k, v in rounds.items()},
        torch_missing=missing or None,
        **floors("gwgrad", mid.numel() * 2 + g.numel() * 4, P * Gr * 16 * 9 * 64),
        **floors("gdgrad", g.numel() * 4 + mid.numel() * 2 + dmid.numel() * 4, P * sum(pk2.couts) * 9 * 64),
        **floors("wgrad1", sh.numel() * 2 + dmid.numel() * 4, P * pc1.cout * 9 * 64),
        gwgrad_needed_product_floor_us=round(2 * P * sum(pk2.couts) * 9 * 64 / MFMA_F32 * 1e6, 2),
        ratio_torch_gwgrad=ratio("torch_gwgrad", "gwgrad"), ratio_torch_gdgrad=ratio("torch_gdgrad", "gdgrad"),
        ratio_torch_wgrad1=ratio("torch_wgrad1", "wgrad1"),
        train_step_over_forward_loss=round(med["train_step"] / med["forward_loss"], 3))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
