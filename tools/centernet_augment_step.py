"""Times the CenterNet training input (det_ops.cn_aug_transform / cn_aug_image = csrc/cnaug.hip) and the chain of graphs.CenterNet from
raw images to gradient, with and without the augmentation, at the shape of configs/centernet/centernet_r18_dcn_train.py -- B = 16,
sources of 480 x 640, 640 x 480 and 427 x 640 padded to 640 x 640, a 512 x 512 input in the stem's layout, colour augmentation on, ten
objects per image -- and prints ONE JSON line (also written to --out).

  transform_ms / image_ms / image_plain_ms / preprocess_ms / torch_ms / chain_augmented_ms / chain_plain_ms (+ *_rounds_ms)
                      median / each of three event-timed rounds of `steps` calls, the rounds of all timed things interleaved
  image               md_cn_aug_image with colour: the grey pass, its finish, the output pass
  image_plain         md_cn_aug_image with colour NULL (the output pass alone)
  preprocess          md_image_preprocess on the same matrices: the same bytes moved without the grey pass and without the per-sample
                      extent -- the yardstick for what the augmentation costs
  torch               the same result composed from torch device ops (a mask for the per-sample extent, F.grid_sample, the grey mean, the
                      three functions selected per sample, the lighting, the normalisation, the padded layout); torch_max_abs_diff: its
                      largest distance from the operator's output
  chain_augmented     CenterNet.train_loss(grad=True): the two ops, the network, md_cn_assign_targets, md_cn_loss_grad
  chain_plain         CenterNet.loss(grad=True) on a ready input and a ready example: the network and md_cn_loss_grad
  image_bytes / image_floor_us / image_floor_share
                      the source pixels of every sample once plus the output once / --tbps (default 6.0 TB/s), and that time as a
                      fraction of the op's time
  equal_to_contract   sample 0 of the device result meets the condition of tests/test_cn_augment_gpu.py against tests/cnaug_contract.py

python tools/centernet_augment_step.py [--steps 20] [--out profiles/centernet_augment_step_b16.json]
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
from minddet.models import Config, build_detector  # noqa: E402
from minddet_amd import det_ops, nn_ops  # noqa: E402
from tests import cnaug_contract as cc  # noqa: E402

DEV = "cuda:0"


def time_calls(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_composition(img, sizes, mat, colour, mean, std, out_hw):
    """md_cn_aug_image from torch device ops, fp32 (not its bits: grid_sample's own arithmetic)"""
    B, Hs, Ws, _ = img.shape
    ho, wo = out_hw
    ys, xs = torch.arange(Hs, device=DEV)[None, :, None], torch.arange(Ws, device=DEV)[None, None, :]
    inside = (ys < sizes[:, 0, None, None]) & (xs < sizes[:, 1, None, None])
    x = (img.permute(0, 3, 1, 2).float() * inside[:, None]).contiguous()
    oy, ox = torch.meshgrid(torch.arange(ho, device=DEV, dtype=torch.float32), torch.arange(wo, device=DEV, dtype=torch.float32), indexing="ij")
    sx = mat[:, 0, None, None] * ox + mat[:, 1, None, None] * oy + mat[:, 2, None, None]
    sy = mat[:, 3, None, None] * ox + mat[:, 4, None, None] * oy + mat[:, 5, None, None]
    grid = torch.stack((2 * sx / (Ws - 1) - 1, 2 * sy / (Hs - 1) - 1), -1)
    v = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True) / 255.0        # [B,3,ho,wo]
    g = (0.114 * v[:, 0] + 0.587 * v[:, 1] + 0.299 * v[:, 2])[:, None]
    gm = g.mean((2, 3), keepdim=True)
    c = colour.float()
    a = [c[:, k, None, None, None] for k in range(3)]
    order = torch.tensor(det_ops.CN_COLOUR_ORDERS, device=DEV)[c[:, 6].long()]                            # [B,3]
    for i in range(3):
        f = order[:, i, None, None, None]
        v = torch.where(f == 0, v * a[0], torch.where(f == 1, a[1] * v + (1 - a[1]) * gm, a[2] * v + (1 - a[2]) * g))
    v = v + c[:, 3:6, None, None]
    v = (v - torch.tensor(mean, device=DEV)[None, :, None, None]) / torch.tensor(std, device=DEV)[None, :, None, None]
    out = torch.zeros((B, ho + 16, wo + 16, 4), dtype=torch.bfloat16, device=DEV)
    out[:, 7:7 + ho, 7:7 + wo, :3] = v.permute(0, 2, 3, 1).to(torch.bfloat16)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tbps", type=float, default=6.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "centernet_augment_step_b16.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("centernet_augment_step: needs the GPU (a time taken anywhere else says nothing)")
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centernet", "centernet_r18_dcn_train.py"))
    model = build_detector(dict(cfg.model), cfg.train_cfg, cfg.test_cfg).to(DEV)
    aug = model.augment_op()
    B, G = args.batch, 10
    rng = np.random.default_rng(args.seed)
    sizes_np = np.array([[(480, 640), (640, 480), (427, 640), (480, 640)][b % 4] for b in range(B)], np.int32)
    img_np = np.full((B, 640, 640, 3), 255, np.uint8)
    for b, (h, w) in enumerate(sizes_np):
        # a smooth image plus noise (a photograph's neighbouring pixels are close; pure noise would be the sampler's easiest case for nobody)
        base = rng.uniform(0, 255, (h // 16 + 2, w // 16 + 2, 3))
        img_np[b, :h, :w] = np.clip(np.kron(base, np.ones((16, 16, 1)))[:h, :w] + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)
    cxy = np.stack([rng.uniform(0, 1, (B, G)) * sizes_np[:, 1:2], rng.uniform(0, 1, (B, G)) * sizes_np[:, 0:1]], -1)
    wh = np.exp(rng.uniform(np.log(16.0), np.log(300.0), (B, G, 2)))
    boxes = torch.from_numpy(np.concatenate([cxy - wh / 2, cxy + wh / 2], -1).astype(np.float32)).to(DEV)
    classes = torch.from_numpy(rng.integers(1, 81, (B, G)).astype(np.int32)).to(DEV)
    img, sizes = torch.from_numpy(img_np).to(DEV), torch.from_numpy(sizes_np).to(DEV)
    draws, colour = aug.draw(sizes, torch.Generator(device=DEV).manual_seed(args.seed))
    kw = dict(rand_crop=aug.rand_crop, scale=aug.scale, shift=aug.shift, flip_prop=aug.flip_prop, input_hw=aug.input_hw, down_ratio=aug.down_ratio)
    out_hw = aug.input_hw

    def transform():
        return det_ops.cn_aug_transform(sizes, draws, **kw)

    mat_in, trans_out, flip_width = transform()
    out = torch.empty((B, out_hw[0] + 16, out_hw[1] + 16, 4), dtype=torch.bfloat16, device=DEV)

    def image():
        return det_ops.cn_aug_image(img, sizes, mat_in, aug.mean, aug.std, out_hw, colour=colour, out=out)

    def image_plain():
        return det_ops.cn_aug_image(img, sizes, mat_in, aug.mean, aug.std, out_hw, colour=None, out=out)

    def preprocess():
        return nn_ops.image_preprocess(img, mat_in, aug.mean, aug.std, out_hw)

    def torch_ops():
        return torch_composition(img, sizes, mat_in.view(B, 6), colour, aug.mean, aug.std, out_hw)

    def chain_augmented():
        return model.train_loss(img, sizes, boxes, classes, draws=draws, colour=colour, grad=True)

    ready_input, ready_example = model.train_example(img, sizes, boxes, classes, draws=draws, colour=colour)
    ready_input = ready_input.clone()

    def chain_plain():
        return model.loss(ready_input, ready_example, grad=True)

    timed = dict(transform=transform, image=image, image_plain=image_plain, preprocess=preprocess, torch=torch_ops, chain_augmented=chain_augmented,
                 chain_plain=chain_plain)
    for fn in timed.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in timed}
    for _ in range(3):
        for k, fn in timed.items():
            rounds[k].append(time_calls(fn, args.steps))
    med = {k: statistics.median(v) for k, v in rounds.items()}

    got = image().clone()
    diff = float((torch_ops().float() - got.float()).abs().max())
    torch.cuda.synchronize()
    got0 = got[:1].view(torch.int16).cpu().numpy().view(np.uint16)
    want0 = cc.image(img_np[:1], sizes_np[:1], mat_in[:1].cpu().numpy(), aug.mean, aug.std, out_hw, col=colour[:1].cpu().numpy(), pad=(7, 9), C=4)
    area = np.zeros(got0.shape, bool)
    area[:, 7:7 + out_hw[0], 7:7 + out_hw[1], :3] = True
    ndiff, worst = cc.bf16_differences(got0[area], want0[area])
    equal = bool(worst <= 1 and ndiff * 10000 <= int(area.sum()) and not got0[~area].any())
    loss = chain_augmented()

    nbytes = int((sizes_np[:, 0].astype(np.int64) * sizes_np[:, 1]).sum()) * 3 + out.numel() * 2
    res = dict(metric="centernet_augment_step", config="centernet_r18_dcn_train", batch=B, source_hw=sizes_np[:4].tolist(), padded_hw=[640, 640],
               input_hw=list(out_hw), objects_per_image=G, steps=args.steps, flipped=int((flip_width > 0).sum()), tbps=args.tbps,
               loss_total=round(float(loss["total"]), 5), num_pos=float(loss["num_pos"]))
    for key in timed:
        res[key + "_ms"] = round(med[key], 4)
        res[key + "_rounds_ms"] = [round(t, 4) for t in rounds[key]]
    res.update(image_bytes=nbytes, image_floor_us=round(nbytes / args.tbps / 1e6, 3), image_floor_share=round(nbytes / args.tbps / 1e9 / med["image"], 5),
               image_plain_floor_share=round(nbytes / args.tbps / 1e9 / med["image_plain"], 5),
               preprocess_floor_share=round(nbytes / args.tbps / 1e9 / med["preprocess"], 5),
               colour_cost_ms=round(med["image"] - med["preprocess"], 4), ops_sum_ms=round(med["transform"] + med["image"], 4),
               augmentation_cost_ms=round(med["chain_augmented"] - med["chain_plain"], 4), image_vs_torch=round(med["torch"] / med["image"], 3),
               torch_max_abs_diff=round(diff, 5), contract_elements_differing=ndiff, contract_elements=int(area.sum()), equal_to_contract=equal)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
