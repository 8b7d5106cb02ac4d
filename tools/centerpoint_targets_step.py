"""Times the CenterPoint training-target assignment (det_ops.cp_assign_targets = md_cp_assign_targets, csrc/cptargets.hip) at the nuScenes
shape of configs/centerpoint/centerpoint_pp_nusc_train.py -- B = 4, six tasks, 128 x 128 maps, max_objs 500, 500 seeded objects per
sample -- and prints ONE JSON line (also written to --out).

  op_ms / op_rounds_ms       median / each of three event-timed rounds of `steps` calls (outputs and workspace reused, as a training loop
                             would), interleaved with the rounds of the fills
  store_floor_us / store_floor_share
                             output bytes / --store-tbps (default 6.0 TB/s: plain coalesced stores to HBM on the MI355X sustain 6.0-6.2)
                             and that time as a fraction of op_ms: the share of the store-bandwidth floor
  fill_ms / fill_share       (not a bandwidth floor: six launches, most of them tiny) the same number of bytes (every output once: B x 786 KB of heat maps plus the rows) written by torch's fill
                             kernels into tensors of the same shapes, same timing: what torch pays to store as much with nothing computed;
                             fill_share = fill_ms / op_ms
  heat_kernel_share          the heat-map kernel's part of the two kernels' device time, from one profiled run of `steps` calls (null
                             with the reason when the profiler gives no kernel rows)
  host_numpy_ms              tests/cp_targets_contract.py (the vectorised numpy restatement of the step, one Python loop over objects) on
                             the same inputs on this host: NOT the reference's own per-object loop, which is not part of this repository
  equal_to_contract          the device result meets the integer / bit-exact conditions of tests/test_cp_targets_gpu.py against it

python tools/centerpoint_targets_step.py [--steps 20] [--out profiles/centerpoint_targets_step_b4.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from minddet.models import Config  # noqa: E402
from minddet_amd import det_ops  # noqa: E402
from tests import cp_targets_contract as ct  # noqa: E402


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


def time_calls(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_shares(fn, reps):
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        t = {}
        for ev in prof.key_averages():
            for name in ("cp_heat_kernel", "cp_slot_kernel"):
                if name in ev.key:
                    t[name] = t.get(name, 0.0) + float(getattr(ev, "device_time_total", 0) or getattr(ev, "cuda_time_total", 0))
        if len(t) != 2 or not all(t.values()):
            return None, None, f"the profiler reported no device time for the two kernels ({sorted(t)})"
        return t["cp_heat_kernel"] / sum(t.values()), {k: round(v / reps, 3) for k, v in t.items()}, None
    except Exception as e:  # the measurement is optional; say why it is missing
        return None, None, f"{type(e).__name__}: {e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--store-tbps", type=float, default=6.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "centerpoint_targets_step_b4.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("centerpoint_targets_step: needs the GPU (a time taken anywhere else says nothing)")
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc_train.py"))
    tg = det_ops.CenterPointTargets.from_config(cfg)
    B, G = args.batch, tg.max_objs
    boxes, classes = inputs(B, G, args.seed)
    gb, gc = torch.from_numpy(boxes).to("cuda:0"), torch.from_numpy(classes).to("cuda:0")
    out = tg(gb, gc)
    kw = dict(tasks=tg.tasks, voxel_size=tg.voxel_size, pc_range=tg.pc_range, out_size_factor=tg.out_size_factor,
              gaussian_overlap=tg.gaussian_overlap, min_radius=tg.min_radius, max_objs=tg.max_objs, feature_map_size=tg.feature_map_size)

    def op():
        return det_ops.cp_assign_targets(gb, gc, out=out, **kw)

    scratch = {k: torch.empty_like(v) for k, v in out.items()}

    def floor():
        for v in scratch.values():
            v.zero_()

    for _ in range(3):
        op()
        floor()
    torch.cuda.synchronize()
    rounds = dict(op=[], floor=[])
    for _ in range(3):
        rounds["op"].append(time_calls(op, args.steps))
        rounds["floor"].append(time_calls(floor, args.steps))
    med = {k: statistics.median(v) for k, v in rounds.items()}

    ncs = det_ops._task_num_classes(tg.tasks)
    ckw = {k: v for k, v in kw.items() if k != "tasks"}
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = ct.assign(boxes, classes, num_classes=ncs, **ckw)
        host.append((time.perf_counter() - t0) * 1e3)
    got = {k: v.cpu().numpy() for k, v in op().items()}
    equal = all(np.array_equal(got[k], want[k]) for k in ("ind", "mask", "cat", "gt_boxes_and_cls")) and \
        np.array_equal(got["hm"] > 0, want["hm"] > 0) and int(ct.bits_apart(got["hm"], want["hm"]).max()) <= 1
    nbytes = sum(v.numel() * v.element_size() for v in out.values())
    res = dict(
        metric="centerpoint_targets_step", config="centerpoint_pp_nusc_train", batch=B, objects_per_sample=G, steps=args.steps,
        drawn=int(got["mask"].sum()), output_bytes=nbytes, heat_map_bytes=out["hm"].numel() * 4,
        op_ms=round(med["op"], 4), op_rounds_ms=[round(t, 4) for t in rounds["op"]],
        store_tbps=args.store_tbps, store_floor_us=round(nbytes / args.store_tbps / 1e6, 3),
        store_floor_share=round(nbytes / args.store_tbps / 1e9 / med["op"], 4), effective_store_gbps=round(nbytes / med["op"] / 1e6, 1),
        fill_ms=round(med["floor"], 4), fill_rounds_ms=[round(t, 4) for t in rounds["floor"]], fill_share=round(med["floor"] / med["op"], 3),
        heat_kernel_share=None, kernels_us_per_call=None, heat_kernel_share_missing="not measured yet",
        host_numpy_ms=round(statistics.median(host), 2), host_numpy_rounds_ms=[round(t, 2) for t in host],
        host_is="tests/cp_targets_contract.py (vectorised numpy restatement), not the reference's per-object loop",
        equal_to_contract=bool(equal))

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(res) + "\n")

    write()                                           # the times are on disk before the profiled run starts
    share, kernels_us, why = kernel_shares(op, args.steps)
    res.update(heat_kernel_share=None if share is None else round(share, 3), kernels_us_per_call=kernels_us, heat_kernel_share_missing=why)
    write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
