"""Times the head training step of CenterNet (optim.CenterNetHeadTrainer: md_cn_loss_grad -> md_conv_bwd_weight (head2, 1x1, three
blocks) -> md_conv1x1_bwd_data (through head1's ReLU) -> md_conv_bwd_weight (head1, 3x3) -> md_adam_step) at the shape of
configs/centernet/centernet_r18_dcn_train.py with the reference's batch -- B = 16, a 128 x 128 x 64 feature map, head1 64 -> 192, head2
192 -> 84 -- on seeded images and boxes through CenterNet.train_example, next to the same gradients from torch on the fp32-widened
operands, and prints ONE JSON line (also written to --out).

  wgrad1_ms, dgrad_ms, wgrad2_ms   md_conv_bwd_weight (3x3, head1), md_conv1x1_bwd_data, md_conv_bwd_weight (1x1, head2): median of three
                                   event-timed rounds of `steps` calls; the rounds of everything timed are interleaved
  adam1_ms, adam2_ms               md_adam_step on the two flat ranges
  train_step_ms / forward_loss_ms  CenterNetHeadTrainer.train_step from the network input against CenterNet.loss(grad=True) alone
  torch_*_ms                       torch.nn.grad.conv2d_weight / conv2d_input (and the ReLU mask) on the operands widened to fp32 inside the
                                   timed region, as a framework step does; null with the reason where torch could not run it
  *_byte_floor_us                  x, dy and dx (or dw's operands) once at 8 TB/s
  *_product_floor_us               the operator's multiply-adds at the fp32 MFMA rate, 157 TFLOP/s
  *_in_bound                       the device result meets the Gaussian-data condition of tests/test_convbwd_gpu.py against the float64
                                   judges (head1's weight gradient: its first 8 output channels)

python tools/centernet_head_train_step.py [--steps 20] [--out profiles/centernet_head_train_step_b16.json]
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
from tests import convbwd_contract as cc, train_contract as tc  # noqa: E402
from tools.pointpillars_loss_step import time_calls  # noqa: E402

HBM, MFMA_F32 = 8e12, 157e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch baselines")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "centernet_head_train_step_b16.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("centernet_head_train_step: needs the GPU (a time taken anywhere else says nothing)")
    dev = "cuda:0"
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centernet", "centernet_r18_dcn_train.py"))
    net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).to(dev)
    B = args.batch
    rng = np.random.default_rng(args.seed)
    img = torch.from_numpy(rng.integers(0, 256, (B, 512, 512, 3)).astype(np.uint8)).to(dev)
    sizes = torch.full((B, 2), 512, dtype=torch.int32, device=dev)
    c, s = rng.uniform(60, 450, (B, 20, 2)), rng.uniform(20, 200, (B, 20, 2))
    boxes = torch.from_numpy(np.concatenate([c - s / 2, c + s / 2], -1).astype(np.float32)).to(dev)
    classes = torch.from_numpy(rng.integers(1, 81, (B, 20)).astype(np.int32)).to(dev)
    inp, ex = net.train_example(img, sizes, boxes, classes, generator=torch.Generator(device=dev).manual_seed(args.seed))
    tr = net.head_trainer()
    o1, o2, pc1, pc2 = tr.opts["head1"], tr.opts["head2"], net.head1.packed, net.head2.packed
    state = {k: o.state() for k, o in tr.opts.items()}
    first = tr.train_step(inp, ex, 5e-4)
    x, h, g = first["x"], first["h"], first["grad"]
    dh = torch.empty_like(first["dh"])
    blocks, n_out = tr.blocks(), net.n_out
    P = x.shape[0] * x.shape[1] * x.shape[2]
    w2_32 = pc2.w.float()[:n_out, :pc2.cin].reshape(n_out, pc2.cin, 1, 1).contiguous()

    def torch_wgrad1():
        return torch.nn.grad.conv2d_weight(x.float().permute(0, 3, 1, 2), (pc1.cout, pc1.cin, 3, 3), dh.permute(0, 3, 1, 2), padding=1), dh.sum((0, 1, 2))

    def torch_wgrad2():
        return torch.nn.grad.conv2d_weight(h.float().permute(0, 3, 1, 2), (n_out, pc2.cin, 1, 1), g.permute(0, 3, 1, 2)[:, :n_out]), g.sum((0, 1, 2))

    def torch_dgrad():
        d = torch.nn.grad.conv2d_input((B, pc2.cin, x.shape[1], x.shape[2]), w2_32, g.permute(0, 3, 1, 2)[:, :n_out])
        return d * (h.permute(0, 3, 1, 2) > 0)

    fns = dict(
        wgrad1=lambda: det_ops.conv_bwd_weight(x, dh, pc1, out=(o1.view("w", "grad"), o1.view("b", "grad"))),
        dgrad=lambda: det_ops.conv1x1_bwd_data(g, pc2, cout=n_out, act=h, out=dh),
        wgrad2=lambda: det_ops.conv_bwd_weight(h, g, pc2, cout=n_out, blocks=blocks, out=(o2.view("w", "grad"), o2.view("b", "grad"))),
        adam1=lambda: o1.step(5e-4, 0.9), adam2=lambda: o2.step(5e-4, 0.9),
        train_step=lambda: tr.train_step(inp, ex, 5e-4), forward_loss=lambda: net.loss(inp, ex, grad=True))
    fns["dgrad"]()
    missing = {}
    if not args.no_torch:
        for name, fn in (("torch_wgrad1", torch_wgrad1), ("torch_dgrad", torch_dgrad), ("torch_wgrad2", torch_wgrad2)):
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
    for k, o in tr.opts.items():
        o.load_state(state[k])

    def write(res):
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(res) + "\n")

    write(dict(metric="centernet_head_train_step", partial=True, **{k + "_ms": round(v, 4) for k, v in med.items()}))   # the times are on disk before the judges run
    # the device results against the float64 judges, on the tensors of one chain
    fns["wgrad2"](), fns["dgrad"](), fns["wgrad1"]()
    torch.cuda.synchronize()
    xn, hn, gn, dhn = x.float().cpu().numpy(), h.float().cpu().numpy(), g.cpu().numpy(), dh.cpu().numpy()
    rows2, kpad2 = pc2.w.shape
    want2 = cc.wgrad_kxk(hn, gn, pc2.cin, n_out, kernel=1, blocks=blocks, rows=rows2, kpad=kpad2)
    e2 = np.abs(o2.view("w", "grad").cpu().numpy().astype(np.float64) - want2["dw"])
    wantd = cc.dgrad_1x1(gn, pc2.w.float().cpu().numpy(), pc2.cin, n_out, act=hn)
    ed = np.abs(dhn.astype(np.float64) - wantd["dx"])
    want1 = cc.wgrad_kxk(xn, dhn, pc1.cin, 8, kernel=3, korder=pc1.korder)
    e1 = np.abs(o1.view("w", "grad").cpu().numpy()[:8].astype(np.float64) - want1["dw"])

    def floors(name, nbytes, macs):
        return {f"{name}_byte_floor_us": round(nbytes / HBM * 1e6, 2), f"{name}_product_floor_us": round(2 * macs / MFMA_F32 * 1e6, 2),
                f"{name}_over_byte_floor": round(med[name] * 1e3 / (nbytes / HBM * 1e6), 2),
                f"{name}_over_product_floor": round(med[name] * 1e3 / (2 * macs / MFMA_F32 * 1e6), 2)}

    res = dict(
        metric="centernet_head_train_step", config="centernet_r18_dcn_train", batch=B, steps=args.steps,
        features_shape=list(x.shape), hidden_shape=list(h.shape), head_grad_shape=list(g.shape), pack1_shape=list(pc1.w.shape),
        pack2_shape=list(pc2.w.shape), korder1=int(pc1.korder), chain_length=tc.chain_length(P),
        **{k + "_ms": round(v, 4) for k, v in med.items()}, rounds_ms={k: [round(t, 4) for t in v] for k, v in rounds.items()},
        torch_missing=missing or None,
        **floors("wgrad1", x.numel() * 2 + dh.numel() * 4, P * pc1.cout * 9 * pc1.cin),
        **floors("dgrad", g.numel() * 4 + h.numel() * 2 + dh.numel() * 4, P * n_out * pc2.cin),
        **floors("wgrad2", h.numel() * 2 + g.numel() * 4, P * n_out * pc2.cin),
        ratio_torch_wgrad1=round(med["torch_wgrad1"] / med["wgrad1"], 2) if "torch_wgrad1" in med else None,
        ratio_torch_dgrad=round(med["torch_dgrad"] / med["dgrad"], 2) if "torch_dgrad" in med else None,
        ratio_torch_wgrad2=round(med["torch_wgrad2"] / med["wgrad2"], 2) if "torch_wgrad2" in med else None,
        train_step_over_forward_loss=round(med["train_step"] / med["forward_loss"], 3),
        wgrad2_in_bound=bool((e2 <= tc.wgrad_bound(P, want2["absdw"])).all()),
        dgrad_in_bound=bool((ed <= cc.dgrad_bound(n_out, wantd["absdx"])).all()),
        wgrad1_in_bound=bool((e1 <= tc.wgrad_bound(P, want1["absdw"])).all()))
    write(res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
