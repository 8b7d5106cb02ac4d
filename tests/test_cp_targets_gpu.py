"""-m gpu: md_cp_assign_targets (det_ops.cp_assign_targets, csrc/cptargets.hip) against the reference's own AssignLabel outputs
(tests/golden/cp_target_vectors.npz) and, for the production shape, against tests/cp_targets_contract.py, which the CPU tests show equal
to the fixture bit for bit.

Conditions per output: ind / mask / cat and the slot placement exact; anno_box columns 0-2 and 6-7 and all of gt_boxes_and_cls bit
for bit; the support of hm and every centre cell (1.0) exact, hm values within 1 fp32 ulp with at most 1 in 10^4 of the non-zero cells
differing at all (two float64 exponentials good to 1 ulp disagree after rounding to fp32 on about 2^-27 of the values; an fp32
evaluation would differ on a large share); the three logs within 4 fp32 ulp of the float64 value (the bound of md_assign_targets' log
targets); sin / cos within max(4 ulp, 2^-24) of the float64 value of the wrapped fp32 heading (2^-24: half the quantum the heading
itself carries near +-pi).  Then: equal results across calls and streams with garbage-filled outputs, the round trip through
md_centerpoint_decode (pins anno_box's column order against the head's channel order), the scratch-pool path (no workspace operand) on
two streams."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import cp_targets_contract as ct
from tests.conftest import has_gpu
from tests.test_cp_targets_cpu import NAMES, fixture_case

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
NUSC = [1, 2, 2, 1, 2, 2]


def run(boxes, classes, ncs, kw, out=None):
    from minddet_amd import det_ops

    return det_ops.cp_assign_targets(torch.from_numpy(np.ascontiguousarray(boxes)).to(DEV), torch.from_numpy(np.ascontiguousarray(classes)).to(DEV),
                                     tasks=[dict(num_class=n) for n in ncs], out=out, **kw)


def to_np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


def check(tag, got, want, classes, ncs):
    """the conditions of the module docstring; prints the measured figures before it asserts"""
    for k in ct.KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
    for k in ("ind", "mask", "cat"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(bits(got["gt_boxes_and_cls"]), bits(want["gt_boxes_and_cls"]))
    for col in (0, 1, 2, 6, 7):
        assert np.array_equal(bits(got["anno_box"][..., col]), bits(want["anno_box"][..., col])), col
    assert not got["anno_box"][want["mask"] == 0].any()                       # unused and skipped slots are zero in every column
    nz = want["hm"] > 0
    apart = ct.bits_apart(got["hm"], want["hm"])
    ndiff, nnz = int((apart > 0).sum()), int(nz.sum())
    rows = ct.slot_rows(want["mask"].shape, classes, ncs)
    worst_log, worst_ratio, worst_trig = ct.transcendental_errors(got["anno_box"], got["mask"], got["gt_boxes_and_cls"], rows)
    print(f"cp_targets[{tag}]: hm non-zero {nnz}, differing {ndiff}, worst {int(apart.max())} ulp; log worst {worst_log:.3f} ulp; "
          f"sin/cos worst {worst_trig:.3f} ulp, {worst_ratio:.3f} of the bound")
    assert np.array_equal(got["hm"] > 0, nz)                                  # support
    assert np.array_equal(got["hm"] == 1.0, want["hm"] == 1.0) and (want["hm"] == 1.0).sum() > 0
    B, T, M = want["mask"].shape
    H, W = want["hm"].shape[-2:]
    b, t, k = np.nonzero(want["mask"])
    assert (got["hm"][b, t, want["cat"][b, t, k], want["ind"][b, t, k] // W, want["ind"][b, t, k] % W] == 1.0).all()   # centre cells
    assert int(apart.max()) <= 1 and ndiff * 10000 <= nnz, (int(apart.max()), ndiff, nnz)
    assert worst_log <= 4.0 and worst_ratio <= 1.0, (worst_log, worst_ratio)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_cases_equal_the_reference(name):
    boxes, classes, ncs, kw, want = fixture_case(name)
    check(name, to_np(run(boxes, classes, ncs, kw)), want, classes, ncs)


@functools.lru_cache(maxsize=None)
def production():
    """B = 2, the nuScenes task table, 128 x 128, max_objs 500, G = 500 seeded rows of which about a tenth are padding"""
    rng = np.random.default_rng(500)
    B, G = 2, 500
    b = np.zeros((B, G, 9), np.float32)
    b[..., 0:2] = rng.uniform(-52.5, 52.5, (B, G, 2))
    b[..., 2] = rng.uniform(-4, 2, (B, G))
    b[..., 3:5] = np.exp(rng.uniform(np.log(0.3), np.log(14.0), (B, G, 2)))
    b[..., 5] = rng.uniform(0.5, 4.0, (B, G))
    b[..., 6:8] = rng.normal(0, 4, (B, G, 2))
    b[..., 8] = rng.uniform(-7.0, 7.0, (B, G))
    c = rng.integers(1, 11, (B, G)).astype(np.int32)
    pad = rng.uniform(size=(B, G)) < 0.1
    c[pad] = np.where(rng.uniform(size=int(pad.sum())) < 0.5, 0, 11)
    b[0, :4, 3] = (0.0, -1.0, 40.0, 1e-3)                                     # degenerate and extreme sizes among the seeded ones
    kw = dict(voxel_size=(0.2, 0.2), pc_range=(-51.2, -51.2), out_size_factor=4, gaussian_overlap=0.1, min_radius=2, max_objs=500,
              feature_map_size=(128, 128))
    want = ct.assign(b, c, num_classes=NUSC, **kw)
    for v in want.values():
        v.setflags(write=False)
    return b, c, kw, want


def test_production_shape_equals_the_contract():
    b, c, kw, want = production()
    assert 0.05 < (want["gt_boxes_and_cls"][..., 9] == 0).mean() < 0.2 and want["mask"].sum() > 700
    check("nusc", to_np(run(b, c, NUSC, kw)), want, c, NUSC)


def test_equal_across_calls_and_streams_and_every_element_written():
    b, c, kw, want = production()
    first = to_np(run(b, c, NUSC, kw))
    shapes = {k: (tuple(v.shape), v.dtype) for k, v in run(b, c, NUSC, kw).items()}

    def garbage():
        out = {k: torch.empty(shp, dtype=dt, device=DEV) for k, (shp, dt) in shapes.items()}
        for v in out.values():
            v.view(torch.uint8).fill_(0xFF)
        return out

    filled = garbage()
    assert all(bool((v.view(torch.uint8) == 0xFF).all()) for v in filled.values())
    again = to_np(run(b, c, NUSC, kw, out=filled))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    o1, o2 = garbage(), garbage()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        r1 = run(b, c, NUSC, kw, out=o1)
    with torch.cuda.stream(s2):
        r2 = run(b, c, NUSC, kw, out=o2)
    r1, r2 = to_np(r1), to_np(r2)
    for k in ct.KEYS:
        for other in (again, r1, r2):
            assert np.array_equal(bits(first[k]), bits(other[k])), k           # (a surviving 0xFF byte would differ from `first`)
    assert np.array_equal(first["ind"], want["ind"])


def test_round_trip_through_the_existing_decode():
    from minddet_amd import _lib, det_ops

    boxes, classes, ncs, kw, want = fixture_case("small")
    got = to_np(run(boxes, classes, ncs, kw))
    B, T, M = got["mask"].shape
    W, H = kw["feature_map_size"]
    per = 12                                                                  # reg 0-1, height 2, dim 3-5, rot 6-7, vel 8-9, hm 10-11
    off = dict(reg=0, height=2, dim=3, rot=6, vel=8, hm=10)
    head = torch.zeros((B, H, W, per * T), dtype=torch.float32)
    a = torch.from_numpy(got["anno_box"])
    cell = 0.8
    drawn = left_out = 0
    rows = ct.slot_rows(got["mask"].shape, classes, ncs)
    results = []
    for t in range(T):
        head[..., per * t + 10:per * t + 10 + ncs[t]] = -8.0
        for b in range(B):
            k = np.flatnonzero(got["mask"][b, t])
            ind = got["ind"][b, t, k]
            y, x = torch.from_numpy(ind // W).long(), torch.from_numpy(ind % W).long()
            v = a[b, t, k]
            # anno_box = (reg 2, height, dim 3, vel 2, rot 2): into the head's channels by name
            for name, cols in (("reg", (0, 1)), ("height", (2,)), ("dim", (3, 4, 5)), ("vel", (6, 7)), ("rot", (8, 9))):
                for i, col in enumerate(cols):
                    head[b, y, x, per * t + off[name] + i] = v[:, col]
            head[b, y, x, per * t + 10 + torch.from_numpy(got["cat"][b, t, k]).long()] = 8.0
    hb = head.to(torch.bfloat16).to(DEV).contiguous()
    n = H * W
    for t in range(T):
        at = det_ops._CenterPointAttrs()
        at.off_reg, at.off_height, at.off_dim, at.off_rot = per * t, per * t + 2, per * t + 3, per * t + 6
        at.off_vel, at.off_hm, at.num_classes = per * t + 8, per * t + 10, ncs[t]
        at.score_threshold, at.out_size_factor = 0.1, float(kw["out_size_factor"])
        for i in range(2):
            at.voxel_size[i], at.pc_range[i] = kw["voxel_size"][i], kw["pc_range"][i]
        for i, lim in enumerate((-1e3, -1e3, -1e3, 1e3, 1e3, 1e3)):
            at.post_center_range[i] = lim
        scores = torch.empty((B, n), dtype=torch.float32, device=DEV)
        labels = torch.empty((B, n), dtype=torch.int32, device=DEV)
        dec = torch.empty((B, n, 9), dtype=torch.float32, device=DEV)
        nms_boxes = torch.empty((B, n, 7), dtype=torch.float32, device=DEV)
        _lib.call("md_centerpoint_decode", [hb, scores, labels, dec, nms_boxes], extra=at)
        torch.cuda.synchronize()
        results.append((scores.cpu().numpy(), labels.cpu().numpy(), dec.cpu().numpy().astype(np.float64)))
    eps = 2.0 ** -8                                                           # one bf16 rounding (8 significant bits): relative 2^-8

    def slack(v, floor=1.0):                                                  # the fp32 evaluation on both sides: 16 ulp at the operand's size
        return 16 * np.spacing(np.float32(max(abs(v), floor)))

    pc = max(abs(kw["pc_range"][0]), abs(kw["pc_range"][1]))
    for t in range(T):
        scores, labels, dec = results[t]
        for b in range(B):
            k = np.flatnonzero(got["mask"][b, t])
            ind = got["ind"][b, t, k]
            u, cnt = np.unique(ind, return_counts=True)
            shared = set(u[cnt > 1].tolist())
            for kk, i in zip(k, ind):
                drawn += 1
                if int(i) in shared:
                    left_out += 1
                    continue
                g = got["gt_boxes_and_cls"][b, rows[b, t, kk]].astype(np.float64)   # x, y, z, w, l, h, rot, vx, vy, class
                an = got["anno_box"][b, t, kk].astype(np.float64)
                d = dec[b, i]
                assert labels[b, i] == got["cat"][b, t, kk] and abs(scores[b, i] - 1 / (1 + math.exp(-8.0))) < 1e-6
                assert abs(d[0] - g[0]) <= eps * abs(an[0]) * cell + slack(g[0], pc), (b, t, kk, d[0], g[0])
                assert abs(d[1] - g[1]) <= eps * abs(an[1]) * cell + slack(g[1], pc), (b, t, kk, d[1], g[1])
                assert abs(d[2] - g[2]) <= eps * abs(g[2]) + slack(g[2])
                for j in range(3):                                            # dim = exp(log w (1 +- 2^-8))
                    assert abs(d[3 + j] - g[3 + j]) <= g[3 + j] * math.expm1(abs(an[3 + j]) * eps) + slack(g[3 + j]), (j, d[3 + j], g[3 + j])
                for j in range(2):
                    assert abs(d[6 + j] - g[7 + j]) <= eps * abs(g[7 + j]) + slack(g[7 + j])
                # atan2(s (1 + e1), c (1 + e2)): |d rot| <= 2 |s c| 2^-8 / (s s + c c) <= 2^-8, compared on the circle
                dr = (d[8] - g[6] + math.pi) % (2 * math.pi) - math.pi
                assert abs(dr) <= 2 * abs(an[8] * an[9]) * eps / (an[8] ** 2 + an[9] ** 2) * (1 + 4 * eps) + slack(math.pi), (d[8], g[6])
    print(f"cp_targets[round trip]: drawn {drawn}, left out (shared cell) {left_out}")
    assert drawn == int(got["mask"].sum()) and drawn > 20 and 4 * left_out <= drawn


def test_scratch_pool_path_on_two_streams_equals_the_workspace_path():
    """no workspace operand: the library's per-stream scratch pool holds the draw lists (det_ops always passes a workspace, so the
    value tests above run the other path); two concurrent streams each take their own pool buffer"""
    from minddet_amd import _lib, det_ops

    boxes, classes, ncs, kw, want = fixture_case("tiles")
    ref = run(boxes, classes, ncs, kw)
    ref_np = to_np(ref)
    at = det_ops._CPTargetsAttrs()
    at.num_tasks = len(ncs)
    for t, nc in enumerate(ncs):
        at.num_classes[t] = nc
    for i in range(2):
        at.voxel_size[i], at.pc_range[i] = kw["voxel_size"][i], kw["pc_range"][i]
    at.out_size_factor, at.gaussian_overlap, at.min_radius = kw["out_size_factor"], kw["gaussian_overlap"], kw["min_radius"]
    gb, gc = torch.from_numpy(boxes).to(DEV), torch.from_numpy(classes).to(DEV)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for _ in streams:
        o = {k: torch.empty_like(v) for k, v in ref.items()}
        for v in o.values():
            v.view(torch.uint8).fill_(0xFF)
        outs.append(o)
    torch.cuda.synchronize()
    for rep in range(2):                                                      # the second round reuses each stream's pool buffer
        for s, o in zip(streams, outs):
            with torch.cuda.stream(s):
                assert _lib.call("md_cp_assign_targets", [gb, gc, o["hm"], o["anno_box"], o["ind"], o["mask"], o["cat"], o["gt_boxes_and_cls"]],
                                 extra=at) == 0
    for o in outs:
        got = to_np(o)
        for k in ct.KEYS:
            assert np.array_equal(bits(got[k]), bits(ref_np[k])), k
    assert np.array_equal(ref_np["ind"], want["ind"]) and np.array_equal(ref_np["mask"], want["mask"])
