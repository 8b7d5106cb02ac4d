"""Times the CenterPoint multi-sweep input (det_ops.cp_sweeps_merge = csrc/cpsweeps.hip) at the shape of
configs/centerpoint/centerpoint_pp_nusc_sweeps.py -- B = 4, ten sweeps of 26 000 points per sample, the key frame first, the nine
past sweeps filtered (radius 1) and transformed -- against the same result written with torch device operators, and prints ONE JSON
line (also written to --out).

  merge_ms / torch_ms (+ *_rounds_ms)
                      median / each of three event-timed rounds of `steps` calls in one process, the rounds of the two interleaved
  torch               per segment: the mask of remove_close, xyz.double() @ R.T + t (a float64 matmul), the cast, the time column;
                      then cat, a cumsum of the kept flags and an index_copy_ into the zeroed output (a dropped row goes to a spare
                      row behind the output), the offsets gathered from the cumsum: no host read, as the operator.  The segment
                      ranges are host integers there (slices), device operands in the operator
  launches_per_call   the operator's, by construction (the three launches of its entry point), not traced
  floor_bytes / floor_us / floor_share
                      the algorithmic traffic -- every input row read once (4 Fin bytes), every output row written once (20 bytes,
                      kept or zero) -- / --tbps (default 6.0 TB/s), and that time as a fraction of merge_ms.  moved_bytes: what this
                      implementation moves (x and y read by the counting pass, the row read again by the scatter pass)
  equal_to_contract   sample 0 of the device result meets tests/cp_sweeps_contract.py; torch_rows_equal: the share of kept rows on
                      which the torch composition gives the operator's bits (its matmul sums in another order)

python tools/centerpoint_sweeps_step.py [--steps 20] [--out profiles/centerpoint_sweeps_step_b4.json]
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
from tests import cp_sweeps_contract as sc  # noqa: E402
from tests.cp_sweeps_cases import pose  # noqa: E402

DEV = "cuda:0"


def frames(B, S, n, seed):
    """B x S frames of n rows, 5-wide: a ring of returns out to 60 m, one row in fifty on the ego vehicle"""
    rng = np.random.default_rng(seed)
    N = B * S * n
    r, a = 60 * np.sqrt(rng.uniform(0, 1, N)), rng.uniform(0, 2 * np.pi, N)
    near = rng.uniform(size=N) < 0.02
    r = np.where(near, rng.uniform(0, 1.2, N), r)
    pts = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-3, 1, N), rng.uniform(0, 255, N), rng.integers(0, 32, N)], 1).astype(np.float32)
    mats = [[None] + [pose(rng) for _ in range(S - 1)] for _ in range(B)]
    lags = [[0.0] + [0.05 * i for i in range(1, S)] for _ in range(B)]
    return pts, [[n] * S for _ in range(B)], mats, lags


def time_calls(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_merge(points, tab, radius):
    """the operator's result with torch device operators, per segment (see the module text) -> (points_out [N,5], offsets [B+1])"""
    N, (B, S) = points.shape[0], tab["seg_flags"].shape
    rows, keep = [], []
    for b in range(B):
        for s in range(S):
            b0, e0 = (int(v) for v in tab["seg_range"][b, s])
            seg = points[b0:e0]
            fl = int(tab["seg_flags"][b, s])
            if fl & 1:
                keep.append(~((seg[:, 0].abs() < radius) & (seg[:, 1].abs() < radius)))
            else:
                keep.append(torch.ones((e0 - b0,), dtype=torch.bool, device=points.device))
            xyz = seg[:, :3]
            if fl & 2:
                m = tab["dev_tf"][b][s]
                xyz = (xyz.double() @ m[:, :3].T + m[:, 3]).float()
            rows.append(torch.cat([xyz, seg[:, 3:4], torch.full((e0 - b0, 1), float(np.float32(tab["time_lag"][b, s])), device=points.device)], 1))
    rows, keep = torch.cat(rows), torch.cat(keep)
    csum = torch.cumsum(keep, 0)
    out = torch.zeros((N + 1, 5), dtype=torch.float32, device=points.device)
    out.index_copy_(0, torch.where(keep, csum - 1, N), rows)
    offsets = torch.cat([csum.new_zeros(1), csum])[tab["dev_bounds"]].int()
    return out[:N], offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--points", type=int, default=26000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tbps", type=float, default=6.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "centerpoint_sweeps_step_b4.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("centerpoint_sweeps_step: needs the GPU (a time taken anywhere else says nothing)")
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc_sweeps.py"))
    merger = det_ops.SweepMerger.from_config(cfg)
    B, S, n = args.batch, merger.nsweeps, args.points
    pts, lengths, mats, lags = frames(B, S, n, args.seed)
    tab = merger.tables(lengths, mats, lags, order=np.random.RandomState(args.seed))
    N = len(pts)
    pool = torch.from_numpy(pts).to(DEV)
    dtab = [torch.from_numpy(tab[k]).to(DEV) for k in ("seg_range", "transforms", "time_lag", "seg_flags")]
    tab["dev_tf"] = torch.from_numpy(tab["transforms"].reshape(B, S, 3, 4)).to(DEV)
    tab["dev_bounds"] = torch.arange(0, B + 1, device=DEV) * (S * n)
    ws_out = torch.empty((N, 5), dtype=torch.float32, device=DEV)

    def merge():
        return det_ops.cp_sweeps_merge(pool, *dtab, radius=merger.radius, out=ws_out)

    def composed():
        return torch_merge(pool, tab, merger.radius)

    timed = dict(merge=merge, torch=composed)
    for fn in timed.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in timed}
    for _ in range(3):
        for k, fn in timed.items():
            rounds[k].append(time_calls(fn, args.steps))
    med = {k: statistics.median(v) for k, v in rounds.items()}

    got, offs, status = (t.cpu().numpy() for t in merge())
    tp, toffs = (t.cpu().numpy() for t in composed())
    kept = int(offs[-1])
    # sample 0 against the contract (its segments lie anywhere in the pool: the contract runs on the whole pool with one sample's table)
    c = sc.merge(pts, tab["seg_range"][:1], tab["transforms"][:1], tab["time_lag"][:1], tab["seg_flags"][:1], merger.radius)
    n0 = int(c["offsets"][1])
    try:
        first = np.zeros_like(c["points"])
        first[:n0] = got[:n0]
        sc.check(first, offs[:2], c, what="sample 0")
        equal = bool(status.tolist() == [0] * B)
    except AssertionError as e:
        print("contract:", e, file=sys.stderr)
        equal = False
    same_rows = float((got[:kept].view(np.uint32) == tp[:kept].view(np.uint32)).all(1).mean()) if np.array_equal(offs, toffs) else 0.0

    fin = pts.shape[1]
    floor = N * fin * 4 + N * 20
    moved = N * 8 + N * 16 + N * 20 + B * S * (8 + 96 + 8 + 4)
    res = dict(metric="centerpoint_sweeps_step", config="centerpoint_pp_nusc_sweeps", batch=B, sweeps=S, points_per_sweep=n, rows_in=N, rows_out=kept,
               point_width=fin, steps=args.steps, tbps=args.tbps, launches_per_call=3, launches_traced=False)
    for key in timed:
        res[key + "_ms"] = round(med[key], 4)
        res[key + "_rounds_ms"] = [round(t, 4) for t in rounds[key]]
    res.update(torch_over_merge=round(med["torch"] / med["merge"], 2), floor_bytes=floor, floor_us=round(floor / args.tbps / 1e6, 3),
               floor_share=round(floor / args.tbps / 1e9 / med["merge"], 5), moved_bytes=moved, equal_to_contract=equal,
               torch_offsets_equal=bool(np.array_equal(offs, toffs)), torch_rows_equal=round(same_rows, 6))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
