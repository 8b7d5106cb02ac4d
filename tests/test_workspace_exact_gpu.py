"""Every wrapper of det_ops hands its kernels exactly the bytes md_<op>_workspace_bytes answers (tests/test_workspace_cpu.py pins those
answers).  Here each covered op runs once at its smallest telling shape with that workspace cut out of the middle of a larger block
filled with 0xA5: the kernels must leave both sides of it untouched, and give byte for byte what the same call gives on the library's
scratch pool.  Every call is a valid call."""
import numpy as np
import pytest
import torch

from minddet_amd import _lib, det_ops
from tests import abi_cases_cn, abi_cases_cploss, abi_cases_pploss
from tests.cp_sweeps_cases import scene
from tests.kitti_io_cases import boxes_as_hulls, scan

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, FILL = 4096, 0xA5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Scratch:
    """stands in for _lib.scratch and _lib.call.  guarded: the answer's bytes between two guard zones; pool: no workspace operand"""

    def __init__(self, monkeypatch):
        self.blocks, self.pool, self.marker, self.call = [], False, torch.empty((16,), dtype=torch.uint8, device=DEV), _lib.call
        monkeypatch.setattr(_lib, "scratch", self.scratch)
        monkeypatch.setattr(_lib, "call", self.strip)

    def scratch(self, op, dims, device):
        if self.pool:
            return self.marker
        n = max(_lib.workspace_bytes(op, *dims), 16)
        block = torch.full((GUARD + n + GUARD,), FILL, dtype=torch.uint8, device=device)
        self.blocks.append((op, tuple(int(d) for d in dims), n, block))
        return block[GUARD:GUARD + n]

    def strip(self, name, tensors, **kw):
        return self.call(name, tensors[:-1] if tensors and tensors[-1] is self.marker else tensors, **kw)

    def both(self, ops, fn):
        """fn() once on guarded workspaces and once on the pool -> the guarded run's outputs, after the checks; ops: the entry points whose
        workspace the call must have asked for, in order"""
        first = len(self.blocks)
        self.pool = False
        got = flat(fn())
        self.pool = True
        want = flat(fn())
        self.pool = False
        torch.cuda.synchronize()
        assert [b[0] for b in self.blocks[first:]] == list(ops)
        for op, dims, n, block in self.blocks[first:]:
            assert block.data_ptr() % 256 == 0
            lo, hi = block[:GUARD], block[GUARD + n:]
            assert bool((lo == FILL).all()) and bool((hi == FILL).all()), (op, dims, n, int((lo != FILL).sum()), int((hi != FILL).sum()))
        assert len(got) == len(want) > 0
        for i, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), (ops, i)
        return got


def flat(out):
    if isinstance(out, dict):
        return [out[k] for k in sorted(out) if out[k] is not None]
    if isinstance(out, torch.Tensor):
        return [out]
    return [t for o in out for t in flat(o)]


@pytest.fixture
def ws(monkeypatch):
    return Scratch(monkeypatch)


def sorted_boxes(rng, B, n):
    """[B,n,4] corner boxes in clusters, so that lists are cut well below n"""
    c = rng.uniform(0, 600, (B, n // 8 + 1, 2)).repeat(8, 1)[:, :n] + rng.normal(0, 3, (B, n, 2))
    wh = rng.uniform(20, 60, (B, n, 2))
    return np.concatenate([c - wh / 2, c + wh / 2], 2).astype(np.float32)


@pytest.mark.parametrize("n", [1023, 1024])        # quota 100: the prefix is 512 boxes, the two-level form and its flags start at n = 1024
def test_nms_aligned_below_and_at_two_prefixes(ws, n):
    boxes = dev(sorted_boxes(np.random.default_rng(n), 2, n))
    mask, idx, num = ws.both(["md_nms_aligned"], lambda: det_ops.nms_aligned(boxes, 0.5, mode=det_ops.NMS_MODE_JIT, max_output=100))
    op, dims, nbytes, _ = ws.blocks[-1]
    assert dims == (2, n, 100) and nbytes == 8 * 2 * n * 16 + (256 if n == 1024 else 0)
    assert 0 < int(num.min()) and int(num.max()) <= 100


def test_nms_rotated(ws):
    rng = np.random.default_rng(3)
    L, n = 2, 300
    b = np.zeros((L, n, 7), np.float32)
    b[..., :2] = rng.uniform(0, 40, (L, n // 4, 2)).repeat(4, 1) + rng.normal(0, 0.3, (L, n, 2))
    b[..., 3:6], b[..., 6] = (1.9, 4.5, 1.7), rng.uniform(-3, 3, (L, n))
    idx, num = ws.both(["md_nms_rotated"], lambda: det_ops.nms_rotated(dev(b), 0.2, det_ops.NMS_ROT_GPU))
    assert ws.blocks[-1][1] == (L, n) and 0 < int(num.min()) <= int(num.max()) < n


def test_topk_segmented_just_above_the_multi_workgroup_threshold(ws):
    L, k, seg = 2, 2, 32769
    scores = torch.rand((L * seg,), device=DEV)
    off = torch.arange(0, (L + 1) * seg, seg, dtype=torch.int32, device=DEV)
    vals, idx, cnt = ws.both(["md_topk_segmented"], lambda: det_ops.topk_segmented(scores, off, k, max_segment=seg))
    assert _lib.lib().md_topk_last_path() == 3 and ws.blocks[-1][1] == (L, k, seg)
    want = torch.topk(scores.reshape(L, seg), k).values
    assert torch.equal(vals, want) and cnt.tolist() == [k, k]
    det_ops.topk_segmented(scores, off, k, max_segment=seg - 1)                        # one score fewer: no workspace is asked for
    assert _lib.lib().md_topk_last_path() != 3 and ws.blocks[-1][0] == "md_topk_segmented" and len(ws.blocks) == 1


@pytest.mark.parametrize("max_voxels", [400, 40])       # B max_voxels = 800 > N = 300 > 80
def test_voxelize_and_anchor_mask(ws, max_voxels):
    rng = np.random.default_rng(7)
    pts = np.concatenate([rng.uniform(-1.6, 1.6, (300, 2)), rng.uniform(-5, 3, (300, 1)), rng.uniform(0, 1, (300, 1))], 1).astype(np.float32)
    offsets = dev(np.array([0, 140, 300], np.int32))
    vs, rg = (0.2, 0.2, 8.0), (-1.6, -1.6, -5.0, 1.6, 1.6, 3.0)
    voxels, coors, num_points, voxel_num = ws.both(["md_voxelize"], lambda: det_ops.voxelize(dev(pts), offsets, vs, rg, 4, max_voxels))
    assert ws.blocks[-1][1] == (300, 2, 256, max_voxels) and 0 < int(voxel_num.min()) and int(voxel_num.max()) <= max_voxels
    anchors = dev(np.concatenate([rng.uniform(-1.6, 0, (37, 2)), rng.uniform(0, 1.6, (37, 2))], 1).astype(np.float32))
    mask, area = ws.both(["md_pp_anchor_mask"],
                         lambda: det_ops.anchors_mask_batched(coors, voxel_num, (16, 16), anchors, vs, rg, 1.0, with_area=True))
    assert ws.blocks[-1][1] == (2, 16, 16) and ws.blocks[-1][2] == 2 * 16 * 16 * 4 and 0 < int(mask.sum()) and float(area.max()) > 1


def test_pc_augment_points(ws):
    from tests.test_pc_augment_gpu import batch3

    s = batch3((0, 300, 40))                       # samples 1 and 2 of the family's three (sample 0 is its empty one): B = 2, N = 340
    pts = dev(np.concatenate(s["points"][1:]))
    d = {k: dev(s[k][1:]) for k in ("boxes", "count", "valid", "loc", "rot", "grot", "glob", "rem", "rem_count", "rem_from")}
    offsets = dev(np.array([0, 300, 340], np.int32))
    _, tf, _ = det_ops.pc_noise_per_object(d["boxes"], d["count"], d["valid"], d["loc"], d["rot"], d["grot"])
    out, offs, owner = ws.both(["md_pc_augment_points"], lambda: det_ops.pc_augment_points(pts, offsets, d["boxes"], d["count"], d["valid"], tf,
                                                                                          d["glob"], d["rem"], d["rem_count"], d["rem_from"]))
    assert ws.blocks[-1][1] == (340, 2, 6, 2) and 0 < int(offs[2]) <= 340 and int((owner >= 0).sum()) > 0


def test_cp_augment(ws):
    from tests.test_cp_augment_gpu import batch3

    s, S = batch3((0, 300, 40)), 5                 # samples 1 and 2 of the family's three, as above
    co = s["cand_offsets"]
    d = {k: dev(s[k][1:]) for k in ("gt_boxes", "gt_count", "gt_classes", "cand_boxes", "cand_classes", "cand_group", "cand_count", "glob")}
    d["cand_count"] = dev(np.array([5, 3], np.int32))
    pts, offsets = dev(s["points"]), dev(np.array([0, 300, 340], np.int32))
    cand_points, cand_offsets = dev(s["cand_points"][co[S]:]), dev(co[S:] - co[S])
    counts, keep = ws.both(["md_cp_aug_count_points"], lambda: det_ops.cp_aug_count_points(pts, offsets, d["gt_boxes"], d["gt_count"], 3))
    assert ws.blocks[-1][1] == (2, 6) and int(counts.sum()) > 0
    (accept,) = ws.both(["md_cp_aug_select"],
                        lambda: det_ops.cp_aug_select(d["gt_boxes"], d["gt_count"], keep, d["cand_boxes"], d["cand_count"], d["cand_group"]))
    assert ws.blocks[-1][1] == (2, 6, S) and 0 < int(accept.sum()) < 2 * S
    out, offs = ws.both(["md_cp_aug_points"],
                        lambda: det_ops.cp_aug_points(pts, offsets, d["glob"], cand_points, cand_offsets, d["cand_boxes"], accept))
    ns = len(s["cand_points"]) - int(co[S])
    assert ws.blocks[-1][1] == (340, ns, 2) and 0 < int(offs[2]) <= 340 + ns


def test_cp_sweeps_merge(ws):
    from tests.test_cp_sweeps_gpu import KEYS

    t = scene(12, [[100, 50, 30], [60, 0, 60]])
    pts, offs, status = ws.both(["md_cp_sweeps_merge"], lambda: det_ops.cp_sweeps_merge(dev(t["points"]), *[dev(t[k]) for k in KEYS], radius=1.0))
    assert ws.blocks[-1][1] == (300, 2, 3) and ws.blocks[-1][2] == 36 and status.tolist() == [0, 0] and 0 < int(offs[2]) <= 300


def test_crop_hulls(ws):
    rng = np.random.default_rng(26)
    pts, hulls = dev(scan(27, 300, reach=45.0)), dev(boxes_as_hulls(rng, 2, 3))
    offsets, count = dev(np.array([0, 140, 300], np.int32)), dev(np.array([3, 2], np.int32))
    out, offs, keep = ws.both(["md_pc_crop_hulls"], lambda: det_ops.crop_hulls(pts, offsets, hulls, count))
    assert ws.blocks[-1][1] == (300, 2, 3) and ws.blocks[-1][2] == 1164 and int(keep.sum()) == int(offs[2]) < 300


def test_cn_aug_image_with_colour_draws(ws):
    rng = np.random.default_rng(4)
    img = dev(rng.integers(0, 256, (2, 8, 12, 3), dtype=np.uint8))
    sizes = dev(np.array([[8, 12], [6, 10]], np.int32))
    mat = dev(np.array([[0.2, 0.0, 0.0, 0.0, 0.15, 0.0], [0.18, 0.02, 0.5, -0.02, 0.12, 0.3]], np.float32))
    colour = dev(np.array([[1.2, 0.8, 1.1, 0.01, -0.02, 0.03, 4, 0], [0.7, 1.3, 0.9, -0.01, 0.0, 0.02, 1, 0]], np.float64))
    (y,) = ws.both(["md_cn_aug_image"], lambda: det_ops.cn_aug_image(img, sizes, mat, (0.4, 0.45, 0.47), (0.28, 0.27, 0.29), (50, 50), colour=colour))
    assert ws.blocks[-1][1] == (2, 50, 50) and ws.blocks[-1][2] == 8 * 2 * (2 + 1) and float(y.float().abs().max()) > 0
    det_ops.cn_aug_image(img, sizes, mat, (0.4, 0.45, 0.47), (0.28, 0.27, 0.29), (50, 50))       # without draws no workspace is asked for
    assert len(ws.blocks) == 1


def gt9(rng, B, G):
    g = np.zeros((B, G, 9), np.float32)
    g[..., 0], g[..., 1] = rng.uniform(-3.0, 6.0, (B, G)), rng.uniform(-3.0, 3.0, (B, G))
    g[..., 3:6], g[..., 8] = rng.uniform(0.8, 3.0, (B, G, 3)), rng.uniform(-3, 3, (B, G))
    return g


def test_centerpoint_targets_and_loss(ws):
    rng = np.random.default_rng(8)
    B, G, M, H, W = 2, 3, 4, 8, 12                                  # the map and the two tasks (1 and 2 classes) of tests/abi_cases_cploss.py
    kw = dict(tasks=[1, 2], voxel_size=(0.2, 0.2), pc_range=(-3.2, -3.2), out_size_factor=4, gaussian_overlap=0.1, min_radius=2, max_objs=M,
              feature_map_size=(W, H))
    boxes, classes = dev(gt9(rng, B, G)), dev(np.array([[1, 2, 3], [3, 0, 1]], np.int32))
    got = ws.both(["md_cp_assign_targets"], lambda: det_ops.cp_assign_targets(boxes, classes, **kw))
    assert ws.blocks[-1][1] == (B, 2, G) and ws.blocks[-1][2] == B * 2 * (G + 1) * 16
    targets = det_ops.cp_assign_targets(boxes, classes, **kw)
    assert int(targets["mask"].sum()) > 0
    head = torch.randn((B, H, W, 24), device=DEV).to(torch.bfloat16)
    at = abi_cases_cploss.loss_attrs()
    for grad in (False, True):
        ws.both(["md_cp_loss"], lambda: det_ops.cp_loss(head, targets, at, grad=grad))
        assert ws.blocks[-1][1] == (B, 2, H, W) and ws.blocks[-1][2] == 8 * B * 2 * (12 + 2)


def test_pointpillars_loss(ws):
    rng = np.random.default_rng(9)
    B, H, W, A = 2, 8, 12, 2
    n = H * W * A
    head = torch.randn((B, H, W, 24), device=DEV).to(torch.bfloat16)
    labels = dev(rng.choice(np.array([-1, 0, 0, 0, 1], np.int32), (B, n)))
    reg, anchors = dev(rng.normal(0, 0.3, (B, n, 7)).astype(np.float32)), dev(rng.uniform(-1, 1, (n, 7)).astype(np.float32))
    at = abi_cases_pploss.loss_attrs()
    for grad in (False, True):
        ws.both(["md_pp_loss"], lambda: det_ops.pp_loss(head, labels, reg, anchors, at, grad=grad))
        assert ws.blocks[-1][1] == (B, H, W, A) and ws.blocks[-1][2] == 40 * B * 2 + 4 * B


def test_centernet_targets_and_loss(ws):
    rng = np.random.default_rng(10)
    B, G, M, H, W = 2, 3, 4, 8, 12
    lo = rng.uniform(0, 6, (B, G, 2))
    boxes = dev(np.concatenate([lo, lo + rng.uniform(1, 5, (B, G, 2))], 2).astype(np.float32))
    classes = dev(np.array([[1, 3, 2], [2, 0, 1]], np.int32))
    kw = dict(num_classes=3, feature_map_size=(W, H), max_objs=M)
    ws.both(["md_cn_assign_targets"], lambda: det_ops.cn_assign_targets(boxes, classes, **kw))
    assert ws.blocks[-1][1] == (B, M) and ws.blocks[-1][2] == 16 * B * M
    targets = det_ops.cn_assign_targets(boxes, classes, **kw)
    assert int(targets["reg_mask"].sum()) > 0
    head = torch.randn((B, H, W, 8), device=DEV).to(torch.bfloat16)
    at = abi_cases_cn.loss_attrs()
    for grad in (False, True):
        ws.both(["md_cn_loss"], lambda: det_ops.cn_loss(head, targets, at, grad=grad))
        assert ws.blocks[-1][1] == (B, 3, H, W) and ws.blocks[-1][2] == 8 * B * (4 + 2 * 2) + 4
