"""GPU: the CenterPoint multi-sweep input (include/minddet_hip_cpsweeps.h) through the C ABI, held to the float64 contract
(tests/cp_sweeps_contract.py: the keep decision, the order, columns 3 and 4, the offsets, the status and the zero tail exact; a
transformed coordinate equal to fp32(v) or inside the interval of the length-4 dot product, at most 1 in 10^4 differing from fp32(v))
-- on the reference's own cases (tests/golden/cp_sweeps_vectors.npz), segment lengths around the workgroup width, ranges out of
memory order, every flag combination, the two device-side errors, a row count that takes the block-count scan to its second pass,
the zero tail, determinism and the call forms, the chain into md_voxelize / forward / the training loss on the tiny config, and the
streaming ring."""
import os

import numpy as np
import pytest
import torch

from tests import cp_sweeps_contract as sc
from tests.abi_cases_cpsweeps import CASES
from tests.conftest import has_gpu
from tests.cp_sweeps_cases import NAMES, case_tables, contract_case, fixture_case, pose, radius, scene

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("seg_range", "transforms", "time_lag", "seg_flags")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(t, r=1.0, workspace=True, out=None):
    """the operator on a dict of host operands -> (points, offsets, status) as device tensors"""
    from minddet_amd import det_ops

    return det_ops.cp_sweeps_merge(dev(t["points"]), *[dev(t[k]) for k in KEYS], radius=r, workspace=workspace, out=out)


def hold(t, what, r=1.0, M=None, **kw):
    """run, then the contract's check -> (the contract's dict, the outputs as numpy)"""
    out = None if M is None else torch.full((M, 5), -7.0, dtype=torch.float32, device=DEV)      # a sentinel the zero tail must overwrite
    pts, offs, status = (x.cpu().numpy() for x in run(t, r, out=out, **kw))
    c = sc.merge(t["points"], t["seg_range"], t["transforms"], t["time_lag"], t["seg_flags"], r, M=M)
    assert status.tolist() == c["status"].tolist(), (what, status.tolist())
    sc.check(pts, offs, c, what=what)
    return c, (pts, offs, status)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_cases_against_the_contract(name):
    t = case_tables(name)
    c, (pts, offs, status) = hold(t, name, radius())
    assert np.array_equal(c["points"], contract_case(name)["points"], equal_nan=True)      # (the contract the CPU test held to the reference)
    assert status.tolist() == [0] * len(fixture_case(name)) and offs[-1] < len(t["points"])
    if name == "plants":                                       # every planted decision: the kept rows are the contract's rows, by their intensities
        n = int(offs[-1])
        assert np.array_equal(pts[:n, 3], t["points"][c["src"], 3]) and len(set(t["points"][c["src"], 3].tolist())) > 20


def test_segment_lengths_around_the_workgroup_width():
    """0, 1, 255, 256, 257, 513 rows; a sample with no rows in the middle of B = 3; a segment in which every row is dropped"""
    lengths = [[0, 1, 255, 256, 257, 513], [0, 0, 0, 0, 0, 0], [257, 300, 0, 1, 256, 2]]
    t = scene(5, lengths)
    b0, e0 = t["seg_range"][2, 1]
    t["points"][b0:e0, :2] *= np.float32(0.05)                # within the radius, every one
    assert (np.abs(t["points"][b0:e0, :2]) < 1).all() and t["seg_flags"][2, 1] == 3
    c, (pts, offs, _) = hold(t, "widths", M=len(t["points"]) + 300)
    assert offs[1] == offs[2] and offs[1] > 0 and offs[3] > offs[2]
    kept = np.zeros(len(t["points"]), bool)
    kept[c["src"]] = True
    assert not kept[b0:e0].any() and kept[t["seg_range"][2, 0, 0]:t["seg_range"][2, 0, 1]].all()      # (segment 0 of a sample is not filtered)
    assert 0 < (~kept).sum() - (e0 - b0) < 400


def test_ranges_out_of_memory_order_with_gaps_and_both_widths():
    t = scene(6, [[250, 300, 250], [40, 0, 60]])
    t["seg_range"] = np.array([[[700, 950], [0, 300], [400, 650]], [[960, 1000], [5, 5], [320, 380]]], np.int32)      # gaps: 300-320, 380-400, 650-700, 950-960
    assert len(t["points"]) == 900
    t["points"] = np.concatenate([t["points"], scene(7, [[100]])["points"]])
    c, (pts, offs, _) = hold(t, "ring order, 5-wide")
    assert c["src"][0] == 700 and not np.isin(np.arange(300, 320), c["src"]).any()
    four = dict(t, points=np.ascontiguousarray(t["points"][:, :4]))
    _, (pts4, offs4, _) = hold(four, "ring order, 4-wide")
    assert sc.same_bits(pts, pts4) and np.array_equal(offs, offs4)


def test_flags_on_the_same_segment():
    """flags 0 / 1 / 2 / 3 over one range; with bit 1 clear xyz passes bit for bit: -0.0, a denormal, a NaN"""
    t = scene(8, [[400], [400], [400], [400]], flags=[[0], [1], [2], [3]])
    t["seg_range"][:] = (100, 500)
    odd = np.array([[-0.0, 5.0, 1e-42], [1e-45, -3.0, -0.0], [np.nan, 0.5, 2.0], [4.0, np.nan, np.nan], [-1e-40, -1e-41, 0.0]], np.float32)
    t["points"][100:105, :3] = odd
    c, (pts, offs, _) = hold(t, "flags")
    n = np.diff(offs)
    assert n[0] == n[2] == 400 and n[1] == n[3] < 400
    assert sc.same_bits(pts[:5, :3], odd) and sc.same_bits(pts[:400, :4], t["points"][100:500, :4])      # flags 0: the input bits
    first = pts[offs[1]:offs[1] + 4, :3]                       # flags 1: row 4 (inside the radius) is gone, rows 0-3 are kept with their bits
    assert sc.same_bits(first, odd[:4])
    for b in range(4):
        assert (pts[offs[b]:offs[b + 1], 4] == np.float32(t["time_lag"][b, 0])).all()


def test_status_of_bad_ranges_and_nothing_faults():
    """a range past N: that sample is empty, the others as without it; a total above N: every sample empty.  The kernels clamp a row
    index before they load, so neither touches memory outside `points`"""
    base = scene(9, [[200, 100], [150, 50], [120, 80]])
    N = len(base["points"])
    _, (good, goffs, _) = hold(base, "in range")
    for k, bad_range in enumerate(((N - 10, N + 1), (-1, 40), (N + 1, N + 1), (5, -3))):
        t = dict(base, seg_range=base["seg_range"].copy())
        t["seg_range"][1, 1] = bad_range
        _, (pts, offs, status) = hold(t, f"bad range {k}")
        assert status.tolist() == [0, 1, 0] and offs[1] == offs[2] == goffs[1]
        assert sc.same_bits(pts[:offs[1]], good[:goffs[1]]) and sc.same_bits(pts[offs[2]:offs[3]], good[goffs[2]:goffs[3]])
    t = dict(base, seg_range=base["seg_range"].copy())
    t["seg_range"][0, 0], t["seg_range"][2, 1] = (0, N), (0, 1)
    _, (pts, offs, status) = hold(t, "more than N rows", M=N + 7)
    assert status.tolist() == [2, 2, 2] and offs.tolist() == [0, 0, 0, 0] and not pts.any()
    t["seg_range"][1, 0] = (0, N + 5)
    _, (pts, offs, status) = hold(t, "both errors")
    assert status.tolist() == [2, 3, 2] and not pts.any()


def test_block_count_scan_second_pass():
    """257 workgroups of rows in one segment: one more than a pass of the one-workgroup scan over the block counts holds, so the last
    workgroup's place comes from the scan's carry (256 x 256 + 1 rows, the smallest count that does this)"""
    t = scene(10, [[256 * 256 + 1]], flags=[[3]], spread=1.5)
    c, (pts, offs, _) = hold(t, "257 blocks")
    assert 0.5 * len(t["points"]) < offs[1] < 0.9 * len(t["points"]) and c["src"][-1] >= 256 * 256 - 8


def test_zero_tail_up_to_m():
    t = scene(11, [[300, 77]])
    for M in (377, 378, 377 + 256 * 9 + 3):
        c, (pts, offs, _) = hold(t, f"M = {M}", M=M)
        assert pts.shape == (M, 5) and offs[1] < 377 and not pts[offs[1]:].any() and pts[:offs[1], 3].all()
    empty = dict(t, seg_range=np.zeros((1, 2, 2), np.int32))
    _, (pts, offs, _) = hold(empty, "nothing kept", M=400)
    assert offs.tolist() == [0, 0] and not pts.any()


def test_bit_identical_across_calls_streams_and_call_forms():
    t = scene(12, [[700, 300, 513], [256, 0, 900]])
    first = run(t)
    again = run(t)
    pool = run(t, workspace=False)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = run(t)
        pool_side = run(t, workspace=False)
    torch.cuda.synchronize()
    for tag, o in (("again", again), ("pool", pool), ("second stream", other), ("pool on the second stream", pool_side)):
        for a, b in zip(first, o):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), tag


def _model():
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_tiny_sweeps.py"))
    return build_detector(dict(cfg.model), dict(cfg.train_cfg), cfg.test_cfg).to(DEV), cfg


def test_chain_into_voxeliser_forward_and_training_loss():
    from minddet_amd import det_ops

    m, cfg = _model()
    rng = np.random.default_rng(13)
    B, S = 2, 3
    lengths = [[900, 700, 800], [600, 850, 750]]
    t = scene(14, lengths, spread=3.0, scale=1.5)
    mats = [[None] + [pose(rng, 1.5) for _ in range(S - 1)] for _ in range(B)]
    mats[1][2] = None                                          # a padding sweep
    lags = [[0.0, 0.05, 0.1], [0.0, 0.05, 0.0]]
    order = [[1, 0], [0, 1]]
    pool = dev(t["points"])
    pts, offs, status = m.merge_sweeps(pool, lengths, mats, lags, order=order, return_status=True)
    tab = m.sweeps_op().tables(lengths, mats, lags, order=order)
    c = sc.merge(t["points"], tab["seg_range"], tab["transforms"], tab["time_lag"], tab["seg_flags"], 1.0)
    assert status.tolist() == [0, 0] and tab["seg_flags"].tolist() == [[0, 3, 3], [0, 3, 1]]
    sc.check(pts.cpu().numpy(), offs.cpu().numpy(), c, what="tiny config")
    want_pts, want_offs = dev(c["points"]), dev(c["offsets"])
    vox_a = det_ops.voxelize(pts, offs, m.voxel_size, m.pc_range, m.max_points, m.max_voxels)
    vox_b = det_ops.voxelize(want_pts, want_offs, m.voxel_size, m.pc_range, m.max_points, m.max_voxels)
    for x, y in zip(vox_a, vox_b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert int(vox_a[3].min()) > 100
    dets, count = m.forward_sweeps(pool, lengths, mats, lags, order=order)
    dets2, count2 = m.forward(want_pts, want_offs)
    assert torch.equal(dets.view(torch.int32), dets2.view(torch.int32)) and torch.equal(count, count2)
    # training: merge_sweeps -> train_loss, device tensors handed on as they are
    G = 4
    boxes = np.zeros((B, G, 9), np.float32)
    for b in range(B):
        for g in range(G):
            boxes[b, g] = (-4.5 + 3 * g, rng.uniform(-3, 3), -1.0, 1.6, 3.2, 1.5, rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-3, 3))
    gt = (dev(boxes), dev(np.tile(np.array([[1, 2, 3, 1]], np.int32), (B, 1))), dev(np.array([4, 3], np.int32)))
    draws = m.augment_op().draw(B, torch.Generator(device=DEV).manual_seed(5))
    one = m.train_loss(*m.merge_sweeps(pool, lengths, mats, lags, order=order), *gt, draws=draws)
    two = m.train_loss(want_pts, want_offs, *gt, draws=draws)
    torch.cuda.synchronize()
    for k in ("total", "parts", "num_pos"):
        assert torch.isfinite(one[k].float()).all() and torch.equal(one[k].view(torch.uint8), two[k].view(torch.uint8)), k
    assert float(one["total"]) > 0 and int(one["example"]["augment"]["counts"].sum()) > 0


def test_sweep_ring_equals_one_merge_of_the_concatenated_frames():
    from minddet_amd import det_ops

    rng = np.random.default_rng(15)
    n_s, slot = 5, 300
    ring = det_ops.SweepRing(n_s, slot, device=DEV)
    frames = [scene(20 + i, [[int(rng.integers(200, slot + 1))]])["points"] for i in range(6)]
    frames[3] = frames[3][:slot]
    poses = [pose(rng, 40.0) for _ in range(6)]
    stamps = [100.0 + 0.05 * i + float(rng.uniform(0, 1e-3)) for i in range(6)]

    def one_call(held):
        """the frames `held` (oldest first) back to back, merged into the newest with one call"""
        inv = np.linalg.inv(poses[held[-1]])
        lens = [len(frames[i]) for i in held]
        end = np.cumsum(lens)
        t = dict(points=np.concatenate([frames[i] for i in held]), seg_range=np.stack([end - lens, end], 1).astype(np.int32)[None],
                 transforms=np.stack([(inv @ poses[i])[:3].reshape(12) for i in held])[None],
                 time_lag=np.array([[stamps[held[-1]] - stamps[i] for i in held]]), seg_flags=np.array([[2] * (len(held) - 1) + [0]], np.int32))
        return hold(t, f"frames {held}", 0.0)[1]

    outs = [ring.push(dev(frames[i]), poses[i], stamps[i]) for i in range(6)]
    data_ptr = ring.buffer.data_ptr()
    for i, held in ((0, [0]), (2, [0, 1, 2]), (4, [0, 1, 2, 3, 4]), (5, [1, 2, 3, 4, 5])):      # the sixth push evicts the oldest
        pts, offs, status = (x.cpu().numpy() for x in outs[i])
        want, woffs, _ = one_call(held)
        n = int(woffs[-1])
        assert status.tolist() == [0] and np.array_equal(offs, woffs) and pts.shape == (n_s * slot, 5)
        assert n == sum(len(frames[k]) for k in held) and sc.same_bits(pts[:n], want[:n]) and not pts[n:].any()
    assert ring.buffer.data_ptr() == data_ptr and [f[0] for f in ring.frames] == [1, 2, 3, 4, 0]
    buf = ring.buffer.cpu().numpy()
    for k, i in ((0, 5), (1, 1), (2, 2), (3, 3), (4, 4)):      # slot k holds frame i: a past frame is where its own push put it
        assert sc.same_bits(buf[k * slot:k * slot + len(frames[i])], frames[i])
    with pytest.raises(ValueError):
        ring.push(dev(np.zeros((slot + 1, 5), np.float32)), poses[0], 101.0)
    assert ring.pushed == 6                                    # the refused frame changed nothing


def test_abi_rows_are_accepted():
    from minddet_amd import _lib

    dt = {"float32": torch.float32, "float64": torch.float64, "int32": torch.int32, "uint8": torch.uint8}
    keep = []
    for c in CASES:
        tensors = [torch.zeros(t.shape, dtype=dt[t.dtype], device=DEV) for t in c.operands]
        keep.append(tensors)
        assert _lib.call(c.sym, tensors, extra=c.extra) == 0, c.id
    torch.cuda.synchronize()
    for tensors in keep:
        assert not tensors[5].any() and not tensors[6].any() and not tensors[7].any()
