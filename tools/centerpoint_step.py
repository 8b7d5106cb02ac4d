"""Times the CenterPoint-PP detector (configs/centerpoint/centerpoint_pp_nusc.py: RPN neck -> CenterHead -> per-task post-processing ->
task merge) on a seeded 512 x 512 x 64 pseudo-image and prints ONE JSON line:

  ms_per_step / samples_per_s   median of three timed rounds of `steps` forward passes (B = batch)
  nonempty_fraction             the fraction of pseudo-image cells that carry a pillar: a modelling choice of this tool, not a nuScenes
                                statistic (the clock depends on the data: the decode's masks and the NMS lists follow the head's values)
  convs                         every conv-family launch of one forward pass, bracketed by HIP events on the launch stream: flops, algorithmic
                                bytes (inputs read once, outputs written once, weights), time and frac_of_roofline = max(flops / MFMA peak,
                                bytes / HBM peak) / time (bench.py's formula); md_conv2d_grouped's flops = 2 N H W sum_g cout_g cin_g k^2
  head                          the head's three launches (shared conv, merged first convs, grouped last convs) from that table
  frac_of_layerwise_roofline    sum over the conv launches of their roofline time / their measured time
  grouped_vs_per_head           the grouped launch against the 36 md_conv2d launches of the per-head form on the same intermediate,
                                interleaved, median of three rounds of `reps` each

python tools/centerpoint_step.py [--batch 4] [--steps 20] [--reps 20] [--nonempty 0.1]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from minddet.models import Config, build_detector  # noqa: E402
from minddet_amd import _lib, nn_ops  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0  # as bench.py
PEAK_HBM_BPS = 8.0e12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def conv_cost(name, tensors, extra):
    """(flops, algorithmic bytes, shape text) of one md_conv2d / md_conv2d_grouped call"""
    if name == "md_conv2d_grouped":
        x, w, b, y = tensors
        n, h, wd, _ = x.shape
        couts = list(extra.cout)[:extra.groups]
        fl = 2.0 * n * h * wd * sum(couts) * extra.cin_g * extra.k * extra.k
        by = 2.0 * n * h * wd * (extra.cin_g * extra.groups + sum(couts)) + 2.0 * w.numel() + 4.0 * b.numel()
        return fl, by, f"grouped G{extra.groups} k{extra.k} {tuple(x.shape)}->{sum(couts)}ch"
    x, w, b, res, y = tensors
    n = x.shape[0]
    cin = extra.x_cin if extra.x_cin else x.shape[3]
    if extra.adv:
        ho, wo, cout = extra.sub_h, extra.sub_w, extra.cout
    else:
        ho, wo, cout = y.shape[1], y.shape[2], y.shape[3]
    fl = 2.0 * n * ho * wo * cout * cin * extra.kh * extra.kw
    by = 2.0 * (x.shape[0] * x.shape[1] * x.shape[2] * cin + n * ho * wo * cout) + 2.0 * w.numel() + 4.0 * b.numel()
    if res is not None:
        by += 2.0 * n * ho * wo * cout
    return fl, by, f"conv {extra.kh}x{extra.kw}/s{extra.stride} {tuple(x.shape)}[{cin}]->{cout}ch {ho}x{wo}"


def instrumented_pass(model, x):
    """one forward pass with every conv-family launch bracketed by events -> list of records"""
    recs = []
    orig = _lib.call

    def call(name, tensors, extra=None, stream=None):
        if name not in ("md_conv2d", "md_conv2d_grouped"):
            return orig(name, tensors, extra, stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = orig(name, tensors, extra, stream)
        e1.record()
        recs.append((name, conv_cost(name, tensors, extra), e0, e1))
        return rc

    _lib.call = call
    try:
        model.forward(x)
    finally:
        _lib.call = orig
    torch.cuda.synchronize()
    out = []
    for name, (fl, by, what), e0, e1 in recs:
        ms = e0.elapsed_time(e1)
        roof = max(fl / (PEAK_BF16_TFLOPS * 1e12), by / PEAK_HBM_BPS) * 1e3
        out.append(dict(op=name, what=what, gflop=round(fl / 1e9, 3), mbytes=round(by / 1e6, 2), us=round(ms * 1e3, 1),
                        bound="mfma" if fl / (PEAK_BF16_TFLOPS * 1e12) >= by / PEAK_HBM_BPS else "hbm",
                        frac_of_roofline=round(roof / ms, 3) if ms > 0 else 0.0, _roof_ms=roof, _ms=ms))
    return out


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
    ap.add_argument("--nonempty", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    dev = "cuda:0"
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc.py"))
    model = build_detector(cfg.model, cfg.train_cfg, cfg.test_cfg).to(dev)
    g = torch.Generator().manual_seed(args.seed)
    B = args.batch
    x = torch.relu(torch.randn((B, 512, 512, 64), generator=g))
    mask = torch.rand((B, 512, 512, 1), generator=g) < args.nonempty
    x = (x * mask).to(torch.bfloat16).to(dev)
    frac = float(mask.float().mean())

    for _ in range(3):
        dets, count = model.forward(x)
    torch.cuda.synchronize()
    rounds = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            model.forward(x)
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) / args.steps * 1e3)
    ms = statistics.median(rounds)

    convs = instrumented_pass(model, x)
    roof = sum(r["_roof_ms"] for r in convs)
    meas = sum(r["_ms"] for r in convs)
    head_recs = convs[-3:]

    # grouped launch vs the 36 per-head md_conv2d launches on the same intermediate, interleaved
    h = model.bbox_head
    feat = model.neck(x)
    sh = h.shared_conv(feat)
    mid = nn_ops.conv2d(sh, h._first)
    y_g = torch.empty((B, 128, 128, 72), dtype=torch.bfloat16, device=dev)
    y_p = torch.empty((B, 128, 128, 8 * len(h.branches())), dtype=torch.bfloat16, device=dev)
    c2s = [c2 for _, _, _, c2 in h.branches()]

    def grouped():
        nn_ops.conv2d_grouped(mid, h._second, y_g)

    def per_head():
        for i, c2 in enumerate(c2s):
            nn_ops.conv2d(mid, c2.packed, out=y_p, c_off=8 * i, x_c_off=64 * i)

    grouped(), per_head()
    torch.cuda.synchronize()
    tg, tp = [], []
    for _ in range(3):
        tg.append(time_calls(grouped, args.reps))
        tp.append(time_calls(per_head, args.reps))
    g_ms, p_ms = statistics.median(tg), statistics.median(tp)
    fl = h._second.flops(B, 128, 128)
    by = 2.0 * B * 128 * 128 * (64 * len(c2s) + sum(h._second.couts)) + 2.0 * h._second.w.numel() + 4.0 * h._second.bias.numel()
    hbm_floor_us = by / PEAK_HBM_BPS * 1e6
    for r in convs:
        r.pop("_roof_ms"), r.pop("_ms")
    print(json.dumps(dict(
        metric="centerpoint_pp_step", batch=B, steps=args.steps, ms_per_step=round(ms, 3), samples_per_s=round(B / ms * 1e3, 1),
        rounds_ms=[round(r, 3) for r in rounds], nonempty_fraction=round(frac, 4), detections=[int(c) for c in count.cpu()],
        frac_of_layerwise_roofline=round(roof / meas, 4), conv_ms=round(meas, 3), convs=convs, head=head_recs,
        grouped_vs_per_head=dict(grouped_us=round(g_ms * 1e3, 1), per_head_36_us=round(p_ms * 1e3, 1), speedup=round(p_ms / g_ms, 2),
                                 grouped_rounds_us=[round(t * 1e3, 1) for t in tg], per_head_rounds_us=[round(t * 1e3, 1) for t in tp],
                                 grouped_gflop=round(fl / 1e9, 3), grouped_mbytes=round(by / 1e6, 1), hbm_floor_us=round(hbm_floor_us, 1),
                                 grouped_frac_of_hbm_roofline=round(hbm_floor_us / (g_ms * 1e3), 3)))))


if __name__ == "__main__":
    main()
