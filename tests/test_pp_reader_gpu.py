"""GPU: md_pp_pillar_encode and md_pp_anchor_mask through the C ABI -- the MFMA operand lane map on exact integer data, the encoder
against the interval contract of tests/pp_reader_contract.py, the batched anchor mask byte for byte against md_anchor_mask per sample,
and the KITTI detector from raw points against the detector on its own pseudo-image and mask.  Outputs sit between guard zones in
sentinel-filled buffers, so stray and missing writes show."""
import os

import numpy as np
import pytest
import torch

from minddet_amd import _lib, det_ops, graphs
from tests import pp_reader_contract as prc
from tests.test_pillars_gpu import Guarded
from tests.test_pp_reader_cpu import CAP, CFG, _detector

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAR = dict(voxel_size=(0.16, 0.16, 4.0), pc_range=(0, -39.68, -3, 69.12, 39.68, 1))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def centre_offsets(voxel_size, pc_range):
    return tuple(float(v) / 2 + float(lo) for v, lo in zip(voxel_size[:3], pc_range[:3]))


def run_encode(voxels, num, coors, voxel_num, reader, hw, voxel_size, offsets):
    """md_pp_pillar_encode into a guarded, sentinel-filled canvas -> the canvas' bytes as int16 [B, H, W, 64] (numpy)"""
    w, scale, shift = reader
    canvas = Guarded((voxels.shape[0], hw[0], hw[1], 64), torch.bfloat16)
    pk = det_ops.PackedPPReader(dev(w), dev(scale), dev(shift))
    t = [x if isinstance(x, torch.Tensor) else dev(x) for x in (voxels, num, coors, voxel_num)]
    det_ops.pp_pillar_encode(*t, pk, hw, voxel_size, offsets, out=canvas.t)
    torch.cuda.synchronize()
    assert canvas.guards_intact(), "a write outside the canvas"
    return canvas.t.view(torch.int16).cpu().numpy()


def bf16_values(bits):
    return torch.from_numpy(bits).view(torch.bfloat16).double().numpy()


def check_encode(bits, lo, hi, live, coors, what):
    """every written cell within the contract's interval, every other cell exactly zero; -> the either-outcome share"""
    got = bf16_values(bits)
    assert not np.isnan(got).any(), f"{what}: cells left unwritten or NaN"
    B, H, W, _ = got.shape
    cb, cy, cx = coors[..., 0], coors[..., 2], coors[..., 3]
    written = live & (cb >= 0) & (cb < B) & (cy >= 0) & (cy < H) & (cx >= 0) & (cx < W)
    b, v = np.nonzero(written)
    g = got[cb[b, v], cy[b, v], cx[b, v]]
    bad = (g < lo[b, v]) | (g > hi[b, v])
    either = float((lo[b, v] != hi[b, v]).mean())
    print(f"{what}: {len(b)} pillars, {int(bad.sum())} of {bad.size} outputs outside the interval, either-outcome share {either:.5f}")
    assert not bad.any(), f"{what}: {int(bad.sum())} outputs outside the interval, first {np.argwhere(bad)[:4].tolist()}"
    assert either < CAP
    empty = np.ones((B, H, W), bool)
    empty[cb[b, v], cy[b, v], cx[b, v]] = False
    assert not bits[empty].any(), f"{what}: a cell without a pillar is not zero"
    return either


# ------------------------------------------------------------------------------------------------------------------- pillar encoder
def test_mfma_operand_lane_map_on_exact_integer_data():
    """integer-valued points, centres and weights: every feature and weight is exact in fp16, every product and every sum exact, so
    the canvas equals an integer computation -- unless a feature column, a k slot or a channel sits in another lane than assumed"""
    rng = np.random.default_rng(7)
    B, MV, MP, H, W = 1, 64, 32, 8, 8
    num = rng.choice([1, 2, 4, 8], MV).astype(np.int32)
    pts = rng.integers(-3, 4, (B, MV, MP, 4)).astype(np.int64) * 8                      # multiples of 8: the mean of 1, 2, 4 or 8 is an integer
    pts[..., 3] = rng.integers(0, 8, (B, MV, MP))
    pts *= (np.arange(MP)[None, None, :, None] < num[None, :, None, None])
    coors = np.zeros((B, MV, 4), np.int64)
    coors[0, :, 1], coors[0, :, 2], coors[0, :, 3] = rng.integers(0, 4, MV), np.arange(MV) // W, np.arange(MV) % W
    w = rng.integers(-2, 3, (64, 10)).astype(np.int64)
    w[:, 0] += 3 * (np.arange(64) % 2)                                                   # (keeps rows and columns apart)
    assert len({tuple(r) for r in w}) == 64 and len({tuple(c) for c in w.T}) == 10       # every channel, every feature column distinguishable
    scale = np.where(np.arange(64) % 3 == 0, -1, 1).astype(np.int64)
    shift = rng.integers(-20, 21, 64).astype(np.int64)
    voxel_size, offsets = (1.0, 2.0, 4.0), (-3.0, 5.0, -2.0)
    # the integer statement
    n = num[None, :, None]
    mean = pts[..., :3].sum(2) // n                                                      # exact: the sums are multiples of 8
    assert (pts[..., :3].sum(2) % n == 0).all()
    ctr = np.stack([coors[..., 3] * 1 - 3, coors[..., 2] * 2 + 5, coors[..., 1] * 4 - 2], -1)
    f = np.concatenate([pts, pts[..., :3] - mean[:, :, None], pts[..., :3] - ctr[:, :, None]], -1)
    f *= (np.arange(MP)[None, None, :, None] < n[..., None])
    assert all(len(np.unique(f[..., k])) > 3 for k in range(10))
    y = np.maximum(scale * (f @ w.T) + shift, 0).max(2)                                  # [B, MV, 64]
    assert np.abs(f @ w.T).max() < 2048 and y.max() < 2048                               # integers an fp16 holds exactly
    want = torch.from_numpy(y.astype(np.float32)).to(torch.bfloat16).view(torch.int16).numpy()
    bits = run_encode(pts.astype(np.float32), num[None], coors.astype(np.int32), np.array([MV], np.int32),
                      (w.astype(np.float32), scale.astype(np.float32), shift.astype(np.float32)), (H, W), voxel_size, offsets)
    got = bits[0].reshape(MV, 64)
    wrong = np.argwhere(got != want[0])
    assert len(wrong) == 0, f"{len(wrong)} of {got.size} differ; channels {sorted(set(wrong[:, 1].tolist()))[:16]}"


@pytest.mark.parametrize("with_distance", [0, 1])
@pytest.mark.parametrize("MP", [20, 32])
def test_encoder_within_the_contract_interval(MP, with_distance):
    hw = (40, 48)
    voxels, num, coors, voxel_num = prc.car_like_voxels(11 + MP + with_distance, B=3, MV=1500, MP=MP, hw=hw, **CAR)
    live = np.arange(1500)[None] < voxel_num[:, None]
    assert {0, 1, MP - 1, MP} <= set(num[0].tolist()) and not live.all() and num[0, 3] == 0
    reader = prc.random_reader(31 + with_distance, K=10 + with_distance)
    assert (reader[2] > 0).any() and (reader[2] < 0).any() and (reader[1] < 0).any()       # padded rows win some maxima; the smallest d some
    off = centre_offsets(CAR["voxel_size"], CAR["pc_range"])
    lo, hi, live = prc.interval(voxels, num, coors, voxel_num, *reader, CAR["voxel_size"], off, bool(with_distance))
    bits = run_encode(voxels, num, coors, voxel_num, reader, hw, CAR["voxel_size"], off)
    check_encode(bits, lo, hi, live, coors, f"MP={MP} with_distance={with_distance}")
    # a live row without points gives relu(fp16(shift)), not zero
    cell = bf16_values(bits)[0, coors[0, 3, 2], coors[0, 3, 3]]
    pad = np.maximum(reader[2].astype(np.float16).astype(np.float64), 0)
    assert np.array_equal(cell, bf16_values(torch.from_numpy(pad).to(torch.bfloat16).view(torch.int16).numpy())) and cell.any()
    again = run_encode(voxels, num, coors, voxel_num, reader, hw, CAR["voxel_size"], off)
    assert again.tobytes() == bits.tobytes(), "a second run differs"


def test_encoder_at_the_car_configs_size_on_voxelised_points():
    """B = 2, 496 x 432, 40 000 rows of 32 points from md_voxelize; the interval is checked on every 16th voxel row (the float64 judge
    of all 80 000 would take half a minute), the zero cells and the repeat on the whole canvas"""
    from tools.pointpillars_points_step import kitti_cloud
    pts, offs = kitti_cloud(2, 60000, seed=5)
    voxels, coors, num, voxel_num = det_ops.voxelize(dev(pts), dev(offs), CAR["voxel_size"], CAR["pc_range"], 32, 40000)
    reader = prc.random_reader(41)
    off = centre_offsets(CAR["voxel_size"], CAR["pc_range"])
    bits = run_encode(voxels, num, coors, voxel_num, reader, (496, 432), CAR["voxel_size"], off)
    vh, ch, nh, vnh = voxels.cpu().numpy(), coors.cpu().numpy(), num.cpu().numpy(), voxel_num.cpu().numpy()
    assert (vnh > 5000).all() and (vnh < 40000).all() and (nh == 32).sum() > 50
    live = np.arange(40000)[None] < vnh[:, None]
    sel = slice(0, None, 16)
    lo, hi, _ = prc.interval(vh[:, sel], nh[:, sel], ch[:, sel], vnh, *reader, CAR["voxel_size"], off)
    sub = bits.copy()
    keep = np.zeros((2, 496, 432), bool)
    b, v = np.nonzero(live[:, sel])
    keep[ch[:, sel][b, v, 0], ch[:, sel][b, v, 2], ch[:, sel][b, v, 3]] = True
    sub[~keep] = 0
    check_encode(sub, lo, hi, live[:, sel], ch[:, sel], "car size, every 16th row")
    occupied = np.zeros((2, 496, 432), bool)
    b, v = np.nonzero(live)
    occupied[ch[b, v, 0], ch[b, v, 2], ch[b, v, 3]] = True
    assert not bits[~occupied].any() and bits[occupied].any(-1).mean() > 0.99
    assert run_encode(voxels, num, coors, voxel_num, reader, (496, 432), CAR["voxel_size"], off).tobytes() == bits.tobytes()


# ---------------------------------------------------------------------------------------------------------------------- anchor mask
@pytest.mark.parametrize("name", ["tiny", "car_xyres16"])
def test_batched_anchor_mask_equals_md_anchor_mask_per_sample(name):
    m = _detector(name + "_points")[0].to(DEV).inner
    H, W = m.grid_hw
    N = m.anchors_bv.shape[0]
    assert name != "car_xyres16" or N == 107136
    B, MV = 3, 256 if name == "tiny" else 40000
    rng = np.random.default_rng(3)
    coors = np.stack([np.broadcast_to(np.arange(B)[:, None], (B, MV)), np.zeros((B, MV), np.int64), rng.integers(0, H, (B, MV)),
                      rng.integers(0, W, (B, MV))], -1).astype(np.int32)
    coors[:, 1::37, 2], coors[:, 2::41, 3], coors[:, 3::43, 2], coors[:, 4::47, 3] = -1, W, H, -5     # outside the grid: not counted
    coors[:, 5::53, 0], coors[:, 5::53, 1] = 9, 3                                                     # b and z are not looked at
    voxel_num = np.array([0, MV // 3, MV], np.int32)
    ct, vt = dev(coors), dev(voxel_num)
    at = det_ops._AnchorMaskAttrs(W, H, m.voxel_size[0], m.voxel_size[1], m.pc_range[0], m.pc_range[1], m.anchor_area_threshold)
    want_area, want_mask = [], []
    for b in range(B):
        a, k = det_ops.anchors_mask(ct[b, :int(voxel_num[b]), 1:].contiguous(), (W, H), m.anchors_bv, m.voxel_size, m.pc_range,
                                    m.anchor_area_threshold)
        want_area.append(a)
        want_mask.append(k.to(torch.uint8))
    want_area, want_mask = torch.stack(want_area), torch.stack(want_mask)
    assert not bool(want_mask[0].any()) and 0 < int(want_mask[1].sum()) < N and int(want_mask[2].sum()) > int(want_mask[1].sum())
    for with_area in (False, True):
        for with_ws in (False, True):
            mask, area, ws = Guarded((B, N), torch.uint8), Guarded((B, N), torch.float32), Guarded((B * H * W * 4,), torch.uint8)
            ops = [ct, vt, m.anchors_bv, mask.t] + ([area.t] if with_area else [None] if with_ws else []) + ([ws.t] if with_ws else [])
            _lib.call("md_pp_anchor_mask", ops, extra=at)
            torch.cuda.synchronize()
            assert mask.guards_intact() and area.guards_intact() and ws.guards_intact()
            assert torch.equal(mask.t, want_mask), (with_area, with_ws)
            if with_area:
                assert torch.equal(area.t.view(torch.int32), want_area.view(torch.int32))
            else:
                assert bool(torch.isnan(area.t).all())
    assert torch.equal(det_ops.anchors_mask_batched(ct, vt, (W, H), m.anchors_bv, m.voxel_size, m.pc_range, m.anchor_area_threshold), want_mask)


def test_batched_anchor_mask_equals_the_numpy_oracle_per_sample():
    """md_anchor_mask and md_pp_anchor_mask run one set of kernels, so the test above compares the code with itself: here the judge is
    oracle/np_ops.anchors_mask (pinned to the reference's fixture by tests/test_oracle_golden.py), area and mask exact.  B = 3 on a
    70 x 5 grid: a row is one full 64-lane chunk and a partial one, so the carry between chunks runs.  The oracle is given what the
    header says is counted (the first voxel_num[b] rows, those inside the grid).  It raises IndexError for an anchor that lies right of
    the grid (c0 >= nx), as the reference does; the device clamps that corner to the last column, so the box is empty: area 0."""
    from oracle import np_ops

    nx, ny, B, MV = 70, 5, 3, 48
    vs, pcr = np.array([0.5, 0.5, 4.0], np.float32), np.array([0.0, -1.25, -3.0, 35.0, 1.25, 1.0], np.float32)
    rng = np.random.default_rng(7)
    coors = np.stack([np.broadcast_to(np.arange(B)[:, None], (B, MV)), np.zeros((B, MV), np.int64), rng.integers(0, ny, (B, MV)),
                      rng.integers(0, nx, (B, MV))], -1).astype(np.int32)
    coors[0, 3, 3], coors[2, 5, 2] = nx, -1                                   # outside the grid, among the counted rows: not counted
    coors[:, :4, 3] = [63, 64, 69, 0]                                         # both sides of the chunk boundary and both ends of a row
    voxel_num = np.array([MV, 0, 17], np.int32)
    bv = np.array([[-10.0, -10.0, 100.0, 100.0],                              # covers everything
                   [-10.0, -1.0, -3.0, 1.0],                                  # entirely left of the grid: c2 < 0 wraps, as numpy's index does
                   [3.0, -0.75, 20.25, 0.5], [30.0, -1.25, 34.25, 1.0], [31.5, 0.0, 32.5, 0.75], [0.0, -1.25, 34.75, 1.0],
                   [40.0, -1.0, 50.0, 1.0]], np.float32)                      # entirely right of the grid (last: the oracle does not take it)
    N = len(bv)
    want_area, want_mask = np.zeros((B, N), np.float32), np.zeros((B, N), np.uint8)
    for b in range(B):
        c = coors[b, :voxel_num[b], 1:]
        c = c[(c[:, 1] >= 0) & (c[:, 1] < ny) & (c[:, 2] >= 0) & (c[:, 2] < nx)]
        a, k = np_ops.anchors_mask(c, (nx, ny), bv[:-1], vs, pcr, 1)
        want_area[b, :-1], want_mask[b, :-1] = a, k
    assert want_area[0, 0] > 20 and not want_area[1].any() and want_mask[2].any() and len(set(want_area[0])) > 4
    at = det_ops._AnchorMaskAttrs(nx, ny, float(vs[0]), float(vs[1]), float(pcr[0]), float(pcr[1]), 1)
    mask, area = Guarded((B, N), torch.uint8), Guarded((B, N), torch.float32)
    _lib.call("md_pp_anchor_mask", [dev(coors), dev(voxel_num), dev(bv), mask.t, area.t], extra=at)
    torch.cuda.synchronize()
    assert mask.guards_intact() and area.guards_intact()
    print("area", area.t.cpu().numpy().tolist(), "want", want_area.tolist())
    assert np.array_equal(area.t.cpu().numpy(), want_area) and np.array_equal(mask.t.cpu().numpy(), want_mask)


# ------------------------------------------------------------------------------------------------------------------------ the model
def small_cloud(m, B, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.array(m.pc_range[:3]), np.array(m.pc_range[3:])
    p = np.concatenate([rng.uniform(lo - 0.2, hi + 0.2, (B * n, 3)), rng.uniform(0, 1, (B * n, 1))], 1).astype(np.float32)
    return p, np.arange(0, (B + 1) * n, n, dtype=np.int32)


@pytest.mark.parametrize("name", ["tiny", "car_xyres16"])
def test_detector_from_points_equals_the_detector_on_its_pseudo_image_and_mask(name):
    from tools.pointpillars_points_step import kitti_cloud
    m = _detector(name + "_points")[0].to(DEV)
    assert type(m) is graphs.PointPillarsKITTIPoints
    if name == "tiny":
        pts, offs = small_cloud(m, 2, 1500, 9)
    else:
        pts, offs = kitti_cloud(2, 60000, seed=2)
    points, offsets = dev(pts), dev(offs)
    (dets, count), aux = m.forward(points, offsets, return_aux=True)
    assert {"voxels", "coors", "num_points", "voxel_num", "pseudo_image", "anchors_mask", "head"} <= set(aux)
    canvas, mask = aux["pseudo_image"], aux["anchors_mask"]
    assert canvas.shape == (2, *m.grid_hw, 64) and canvas.dtype == torch.bfloat16 and mask.dtype == torch.uint8
    assert 0 < int(mask.sum()) < mask.numel() and bool(canvas.any()) and int(aux["voxel_num"].min()) > 0
    # the model the tree had, from the plain config with the same seed: the same weights, fed what the front end made
    from tests.test_pointpillars_cpu import _detector as plain_detector
    old = plain_detector(name)[0].to(DEV)
    assert type(old) is graphs.PointPillarsNet
    want_mask = old.anchors_mask_from_coors(aux["coors"], aux["voxel_num"])
    assert torch.equal(mask, want_mask)
    dets_b, count_b = old.forward(canvas, want_mask)
    assert torch.equal(dets.view(torch.int32), dets_b.view(torch.int32)) and torch.equal(count, count_b)
    dets2, count2 = m.forward(points, offsets)
    assert torch.equal(dets.view(torch.int32), dets2.view(torch.int32)) and torch.equal(count, count2)
    post = m.test_cfg["nms_post_max_size"]
    assert dets.shape == (2, post, 9) and count.shape == (2,) and count.dtype == torch.int32
    if name == "tiny":
        assert int(count.min()) > 0
        from minddet.models import Config, build_detector
        cfg = Config.fromfile(CFG[name + "_points"])
        two = build_detector(dict(cfg.model), cfg.train_cfg, dict(cfg.test_cfg, streams=2)).to(DEV)
        assert two.inner.streams == 2
        d2, c2 = two.forward(points, offsets)
        torch.cuda.synchronize()
        assert torch.equal(dets.view(torch.int32), d2.view(torch.int32)) and torch.equal(count, c2)
        with pytest.raises(ValueError):
            m.forward(torch.cat([points, points[:, :1]], 1), offsets)
        with pytest.raises(ValueError):
            m.forward(points[:, :3].contiguous(), offsets)
