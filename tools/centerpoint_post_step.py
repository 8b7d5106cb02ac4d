"""Times the post-processing of the CenterPoint-PP detector (configs/centerpoint/centerpoint_pp_nusc.py) both ways in ONE process and
prints ONE JSON line (also written to --out): the chain of det_ops.CenterHeadPostBatched (seven launches for every task and sample)
against the parent path, one det_ops.CenterHeadPost per task + graphs.merge_center_tasks, selected by the detector's `cp_post`
argument so that the rounds interleave.  Seeded 512 x 512 x 64 pseudo-image, random weights; B = 4 and B = 1.

Per batch size:
  step_chain_ms / step_per_task_ms   median of three event-timed rounds of `steps` forward passes, rounds of the two forms interleaved
  post_chain_ms / post_per_task_ms   the post-processing alone on the step's own (fixed) head tensor, same timing
  *_rounds_ms                        the rounds; spread = (max - min) over the rounds of both forms
  launches                           per form: calls into the library, the kernel launches those calls make (table below: what each entry
                                     point enqueues at these shapes), and the torch operators dispatched next to them (each at least one
                                     launch; counted by a dispatch mode, not on the hardware)
  faster                             the chain's step is faster than the per-task step by more than the spread of the rounds
`chain_faster_at_both` = `faster` at both batch sizes, `reason` says what was seen.  The chain is selected with MD_CP_POST=1 (or
cp_post=True in the model's config); the detector's default stays the per-task path, whose operator set the production-replay tests pin.
Not measured here: the kernels' own times, and real checkpoints (random weights fill every candidate list: the expensive case of the NMS).

python tools/centerpoint_post_step.py [--steps 20] [--nonempty 0.1] [--out profiles/centerpoint_post_step_b4.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from minddet.models import Config, build_detector  # noqa: E402
from minddet_amd import _lib, det_ops, graphs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel launches per library call at the shapes of this model (16 384 cells per segment: the LDS-staged top-k, one launch)
LAUNCHES = {"md_centerpoint_decode": 1, "md_topk_segmented": 1, "md_gather_rows": 1, "boxes_iou_nms_gpu": 3, "md_cp_scores": 1,
            "md_cp_decode_selected": 1, "md_nms_rotated": 3, "md_cp_pack": 1}


class CountOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = func.overload_packet.__name__ if hasattr(func, "overload_packet") else str(func)
        if name not in ("view", "_unsafe_view", "reshape", "expand", "unsqueeze", "squeeze", "slice", "select", "alias", "detach", "t",
                        "transpose", "permute", "as_strided", "empty", "empty_like", "empty_strided", "unbind", "split", "_reshape_alias"):
            self.n += 1
        return func(*args, **(kwargs or {}))


def count_launches(fn):
    calls = []
    real = _lib.call

    def spy(name, tensors, extra=None, stream=None):
        calls.append(name)
        return real(name, tensors, extra=extra, stream=stream)

    _lib.call = spy
    try:
        with CountOps() as ops:
            fn()
    finally:
        _lib.call = real
    torch.cuda.synchronize()
    return dict(library_calls=len(calls), library_launches=sum(LAUNCHES[c] for c in calls), torch_ops=ops.n)


def time_calls(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(chain, per_task, B, steps, nonempty, seed):
    dev = "cuda:0"
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn((B, 512, 512, 64), generator=g))
    occ = torch.rand((B, 512, 512, 1), generator=g) < nonempty
    x = (x * occ).to(torch.bfloat16).to(dev)
    head, _ = chain.bbox_head(chain.neck(x))
    head = head.clone()
    h = chain.bbox_head
    posts = [det_ops.CenterHeadPost(off, nc, chain.test_cfg) for off, nc in zip(h.task_offsets(), h.num_classes)]

    def step_chain():
        return chain.forward(x)

    def step_per_task():
        return per_task.forward(x)

    def post_chain():
        return chain.post_batched()(head)

    def post_per_task():
        return graphs.merge_center_tasks([p(head) for p in posts], h.num_classes, chain.max_per_task)

    fns = dict(step_chain=step_chain, step_per_task=step_per_task, post_chain=post_chain, post_per_task=post_per_task)
    for _ in range(3):
        outs = {k: f() for k, f in fns.items()}
    torch.cuda.synchronize()
    same = all(torch.equal(outs[k][0], outs["step_chain"][0]) and torch.equal(outs[k][1], outs["step_chain"][1]) for k in fns)
    rounds = {k: [] for k in fns}
    for _ in range(3):
        for k, f in fns.items():
            rounds[k].append(time_calls(f, steps))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    step_all = rounds["step_chain"] + rounds["step_per_task"]
    spread = max(max(rounds[k]) - min(rounds[k]) for k in ("step_chain", "step_per_task"))
    out = dict(batch=B, results_equal=same, detections=[int(c) for c in outs["step_chain"][1].cpu()],
               launches=dict(chain=count_launches(post_chain), per_task=count_launches(post_per_task)),
               step_spread_ms=round(spread, 4), step_range_ms=[round(min(step_all), 3), round(max(step_all), 3)],
               faster=bool(med["step_per_task"] - med["step_chain"] > spread),
               post_ratio=round(med["post_per_task"] / med["post_chain"], 2),
               nonempty_fraction=round(float(occ.float().mean()), 4))
    for k in fns:
        out[k + "_ms"] = round(med[k], 4)
        out[k + "_rounds_ms"] = [round(t, 4) for t in rounds[k]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--nonempty", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "centerpoint_post_step_b4.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("centerpoint_post_step: needs the GPU (a time taken anywhere else says nothing)")
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc.py"))
    chain = build_detector(dict(cfg.model, cp_post=True), cfg.train_cfg, cfg.test_cfg).to("cuda:0")
    per_task = build_detector(dict(cfg.model, cp_post=False), cfg.train_cfg, cfg.test_cfg).to("cuda:0")
    res = [measure(chain, per_task, B, args.steps, args.nonempty, args.seed) for B in (4, 1)]
    ok = all(r["faster"] and r["results_equal"] for r in res)
    reason = ("the chain's step is faster than the per-task step by more than the spread of the rounds at B = 4 and B = 1" if ok else
              "not faster by more than the spread of the rounds at " + ", ".join(f"B = {r['batch']}" for r in res if not r["faster"]))
    line = json.dumps(dict(metric="centerpoint_post_step", config="centerpoint_pp_nusc", steps=args.steps, weights="random",
                           chain_faster_at_both=ok, default="per-task path; MD_CP_POST=1 selects the chain", reason=reason, b4=res[0], b1=res[1]))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
