"""GPU: md_voxelize and md_pillar_encode through the C ABI against the reference fixture (bit-exact), against the numpy / float64
statements of tests/pillar_contract.py (production size; the derived bound), and the detector from raw points against the detector on
its own pseudo-image.  Every output sits between guard zones in a sentinel-filled buffer, so stray and missing writes show.

Measured on an MI355X (this file, `-s` prints the figures): the worst |result - float64| / bound of md_pillar_encode, before the bf16
store's own half ulp, is listed in the commit that introduced the file."""
import os

import numpy as np
import pytest
import torch

from minddet_amd import _lib, det_ops, graphs
from tests import pillar_contract as pc
from tests.test_pillars_cpu import CFG, GOLD, OUT, fixture_case, random_pfn, random_voxels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096
NUSC = dict(voxel_size=(0.2, 0.2, 8.0), pc_range=(-51.2, -51.2, -5.0, 51.2, 51.2, 3.0))


class Guarded:
    """a tensor inside a sentinel-filled buffer with a guard zone on either side"""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape))
        self.sentinel = float("nan") if dtype.is_floating_point else (0xA5 if dtype == torch.uint8 else -7777)
        self.buf = torch.full((n + 2 * GUARD,), self.sentinel, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)

    def guards_intact(self):
        g = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]])
        return bool(torch.isnan(g).all()) if self.buf.dtype.is_floating_point else bool((g == self.sentinel).all())


def run_voxelize(points, offsets, voxel_size, pc_range, max_points, max_voxels):
    """md_voxelize into guarded, sentinel-filled outputs -> 4 numpy arrays"""
    B, F = len(offsets) - 1, points.shape[1]
    p = torch.from_numpy(np.ascontiguousarray(points)).to(DEV)
    off = torch.from_numpy(np.asarray(offsets, np.int32)).to(DEV)
    outs = [Guarded((B, max_voxels, max_points, F), torch.float32), Guarded((B, max_voxels, 4), torch.int32),
            Guarded((B, max_voxels), torch.int32), Guarded((B,), torch.int32)]
    at = det_ops._VoxelizeAttrs()
    for k in range(3):
        at.voxel_size[k] = float(voxel_size[k])
    for k in range(6):
        at.range[k] = float(pc_range[k])
    at.max_points, at.max_voxels = max_points, max_voxels
    gx, gy, gz = det_ops.voxel_grid(voxel_size, pc_range)
    ws = Guarded((det_ops.voxelize_workspace_bytes(len(points), B, gx * gy * gz, max_voxels),), torch.uint8)
    _lib.call("md_voxelize", [p, off] + [o.t for o in outs] + [ws.t], extra=at)
    torch.cuda.synchronize()
    assert all(o.guards_intact() for o in outs), "a write outside an output"
    assert ws.guards_intact(), "a write outside the workspace"
    return [o.t.cpu().numpy() for o in outs]


def assert_same(got, want, what):
    for g, w, k in zip(got, want, OUT):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k)
        assert g.tobytes() == w.tobytes(), f"{what}: {k} differs in {int((g != w).sum())} elements"   # bytes: -0.0 and sentinels count


@pytest.mark.parametrize("name", ["capped", "uncapped", "f4"])
def test_voxelize_equals_the_reference_fixture_bit_for_bit(name):
    z = np.load(GOLD)
    args = fixture_case(z, name)
    got = run_voxelize(*args)
    assert_same(got, [z[name + k] for k in OUT], name)
    assert_same(run_voxelize(*args), got, name + " (second run)")       # deterministic: one repeat, same bytes


def production_cloud(B=4, n=260000):
    from tools.centerpoint_points_step import sweep_cloud
    return sweep_cloud(B, n, seed=3)


@pytest.mark.parametrize("max_voxels", [60000, 20000])
def test_voxelize_at_production_size(max_voxels):
    pts, off = production_cloud()
    want = pc.voxelize_ref(pts, off, NUSC["voxel_size"], NUSC["pc_range"], 20, max_voxels)
    uncapped = pc.voxelize_ref(pts, off, NUSC["voxel_size"], NUSC["pc_range"], 1, 262144)[3]
    print("voxels per sample", uncapped, "cap", max_voxels, "full voxels", int((want[2] == 20).sum()))
    assert ((uncapped > max_voxels) == (max_voxels == 20000)).all()      # 20 000 is below the cloud's voxel count, 60 000 above
    assert (want[2] == 20).sum() > 1000 and (want[2] == 1).sum() > 10000
    got = run_voxelize(pts, off, NUSC["voxel_size"], NUSC["pc_range"], 20, max_voxels)
    assert_same(got, want, f"production, max_voxels {max_voxels}")
    if max_voxels == 60000:
        assert_same(run_voxelize(pts, off, NUSC["voxel_size"], NUSC["pc_range"], 20, max_voxels), got, "second run")


def small_cloud(n, F, seed):
    rng = np.random.default_rng(seed)
    p = np.zeros((n, F), np.float32)
    p[:, :2] = rng.uniform(-7.0, 7.0, (n, 2))
    p[:, 2] = rng.uniform(-5.5, 3.5, n)
    p[:, 3:] = rng.uniform(0, 1, (n, F - 3))
    return p


SMALL = dict(voxel_size=(0.4, 0.4, 2.0), pc_range=(-6.4, -6.4, -5.0, 6.4, 6.4, 3.0))


@pytest.mark.parametrize("F", [4, 5])
def test_voxelize_batch_shapes_and_dropped_points(F):
    p = small_cloud(5000, F, 11)
    for col, v in ((0, np.nan), (1, np.inf), (2, -np.inf), (2, np.nan), (0, -np.inf)):      # non-finite coordinates are dropped
        p[np.arange(7 + col, 5000, 97 + 10 * col), col] = v
    p[5::211, 3] = np.nan                                                                   # a non-finite FEATURE is just data
    cases = {"B=1": [0, 5000], "ragged": [0, 1700, 1701, 4200, 5000], "empty sample": [0, 2000, 2000, 5000], "empty first": [0, 0, 5000],
             "points outside every sample": [300, 2500, 4000]}
    for what, off in cases.items():
        for mv in (4000, 300):
            want = pc.voxelize_ref(p, off, SMALL["voxel_size"], SMALL["pc_range"], 4, mv)
            assert_same(pc.voxelize_loop(p, off, SMALL["voxel_size"], SMALL["pc_range"], 4, mv), want, what + " (statements)")
            assert_same(run_voxelize(p, off, SMALL["voxel_size"], SMALL["pc_range"], 4, mv), want, f"{what}, max_voxels {mv}")
    empty = run_voxelize(p[:0], [0, 0], SMALL["voxel_size"], SMALL["pc_range"], 4, 16)           # no points at all
    assert all(not e.any() for e in empty)


# ------------------------------------------------------------------------------------------------------------------- pillar encoder
def run_encode(voxels, num, coors, voxel_num, pk, hw, at):
    B = voxels.shape[0]
    canvas = Guarded((B, hw[0], hw[1], 64), torch.bfloat16)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    pk = pk.to(DEV)
    det_ops.pillar_encode(t(voxels), t(num), t(coors), t(voxel_num), pk, hw, *at, out=canvas.t)
    torch.cuda.synchronize()
    assert canvas.guards_intact()
    return canvas.t.float().cpu().numpy().astype(np.float64)


def check_encode(voxels, num, coors, voxel_num, layers, hw, at, what):
    """-> worst |got - float64| / (bound + half a bf16 ulp): every live cell within the admissible bf16 interval, all others exactly 0"""
    pk = det_ops.pack_pfn(layers)
    np_ = lambda x: None if x is None else x.cpu().numpy()
    got = run_encode(voxels, num, coors, voxel_num, pk, hw, at)
    feat, bound, live = pc.pfn_ref(voxels, num, coors, voxel_num, np_(pk.w1), np_(pk.b1), np_(pk.w2), np_(pk.b2), *at)
    assert not np.isnan(got).any(), f"{what}: cells left unwritten"
    b, v = np.nonzero(live)
    cb, cy, cx = coors[b, v, 0], coors[b, v, 2], coors[b, v, 3]
    g = got[cb, cy, cx]
    lo, hi = pc.bf16_interval(feat[b, v], bound[b, v])
    bad = (g < lo) | (g > hi)
    half_ulp = np.abs(pc.bf16_round(feat[b, v])) * 2.0 ** -8
    ratio = np.abs(g - feat[b, v]) / (bound[b, v] + half_ulp + 1e-30)
    fp32_ratio = float((np.maximum(0, np.abs(g - feat[b, v]) - half_ulp) / bound[b, v]).max())
    print(f"{what}: {len(b)} pillars, worst |err| / (bound + bf16 half ulp) = {ratio.max():.4f}, worst (|err| - half ulp) / bound = "
          f"{fp32_ratio:.4f}, largest bound = {bound[b, v].max():.3e}")
    assert not bad.any(), f"{what}: {int(bad.sum())} values outside the bound, worst ratio {ratio.max():.3f}"
    empty = np.ones(got.shape[:3], bool)
    empty[cb, cy, cx] = False
    assert not got[empty].any(), f"{what}: a cell without a pillar is not zero"
    return ratio.max()


@pytest.mark.parametrize("two", [False, True], ids=["one-layer", "two-layer"])
@pytest.mark.parametrize("F", [4, 5])
@pytest.mark.parametrize("positive_shift", [False, True], ids=["shift-", "shift+"])
def test_pillar_encode_within_the_derived_bound(two, F, positive_shift):
    hw = (48, 40)
    voxels, num, coors, voxel_num = random_voxels(21 + F, B=3, MV=1500, MP=20, F=F, hw=hw)
    assert {1, 19, 20} <= set(num[0].tolist())
    layers = random_pfn(31, F=F, two=two, positive_shift=positive_shift)
    vx, vy = 0.2, 0.25
    # coordinates like a cloud's: points inside their pillar
    rng = np.random.default_rng(5)
    live_rows = (np.arange(20)[None, None, :] < num[..., None])
    voxels[..., 0] = (coors[..., 3:4] * np.float32(vx) - 4.0 + rng.uniform(0, vx, voxels.shape[:3])) * live_rows
    voxels[..., 1] = (coors[..., 2:3] * np.float32(vy) - 6.0 + rng.uniform(0, vy, voxels.shape[:3])) * live_rows
    voxels = voxels.astype(np.float32)
    check_encode(voxels, num, coors, voxel_num, layers, hw, (vx, vy, vx / 2 - 4.0, vy / 2 - 6.0), f"F={F} two={two} shift+={positive_shift}")
    if positive_shift:       # the case exists to let padded rows win the maximum: they do
        pk = det_ops.pack_pfn(layers)
        assert (pk.b1 > 0).any() and (pk.b1 < 0).any()


def test_pillar_encode_on_voxelised_production_cloud_and_known_shapes():
    """the two ops chained at production size (B = 4, 512 x 512, 20 rows, the config's two-layer net), and the shapes of the reference's
    self-test (pillar_encoder.py:231-253): 1002 zero voxels of 20 x 5 -> a [4, 512, 512, 64] canvas"""
    from minddet.models import Config, build_detector
    cfg = Config.fromfile(CFG)
    m = build_detector(dict(cfg.model), cfg.train_cfg, cfg.test_cfg)
    pts, off = production_cloud(n=120000)
    vox = pc.voxelize_ref(pts, off, NUSC["voxel_size"], NUSC["pc_range"], 20, 60000)
    at = (m.reader.vx, m.reader.vy, m.reader.x_offset, m.reader.y_offset)
    check_encode(vox[0], vox[2], vox[1], vox[3], m.reader.layers, (512, 512), at, "production cloud")
    voxels = np.zeros((4, 1002, 20, 5), np.float32)
    num = np.zeros((4, 1002), np.int32)
    num[0] = 1
    coors = np.zeros((4, 1002, 4), np.int32)
    coors[0, :, 2], coors[0, :, 3] = np.arange(1002) // 512 + 7, np.arange(1002) % 512
    got = run_encode(voxels, num, coors, np.array([1002, 0, 0, 0], np.int32), det_ops.pack_pfn(m.reader.layers), (512, 512), at)
    assert got.shape == (4, 512, 512, 64) and int(got.any(-1).sum()) == 1002 and not got[1:].any()
    check_encode(voxels, num, coors, np.array([1002, 0, 0, 0], np.int32), m.reader.layers, (512, 512), at, "known-answer shapes")


# ------------------------------------------------------------------------------------------------------------------------ the model
def test_detector_from_points_equals_the_detector_on_its_pseudo_image():
    from minddet.models import Config, build_detector
    cfg = Config.fromfile(CFG)
    m = build_detector(dict(cfg.model), cfg.train_cfg, cfg.test_cfg).to(DEV)
    assert type(m) is graphs.PillarDetector
    pts, off = production_cloud(B=2, n=150000)
    points, offsets = torch.from_numpy(pts).to(DEV), torch.from_numpy(off).to(DEV)
    (dets, count), aux = m.forward(points, offsets, return_aux=True)
    assert {"voxels", "coors", "num_points", "voxel_num", "pseudo_image", "head"} <= set(aux)
    canvas = aux["pseudo_image"]
    assert canvas.shape == (2, 512, 512, 64) and canvas.dtype == torch.bfloat16
    want = pc.voxelize_ref(pts, off, NUSC["voxel_size"], NUSC["pc_range"], 20, 60000)
    assert_same([aux[k].cpu().numpy() for k in ("voxels", "coors", "num_points", "voxel_num")], want, "detector's voxels")
    dets_b, count_b = m.detector.forward(canvas)
    assert torch.equal(dets, dets_b) and torch.equal(count, count_b)
    dets2, count2 = m.forward(points, offsets)
    assert torch.equal(dets, dets2) and torch.equal(count, count2)
    T = len(m.bbox_head.num_classes)
    assert dets.shape == (2, T * 83, 11) and dets.dtype == torch.float32 and count.shape == (2,) and count.dtype == torch.int32
    d, c = dets.cpu().numpy(), count.cpu().numpy()
    # (an untrained head can overflow exp() in the box sizes: those columns are only required not to be NaN)
    assert not np.isnan(d).any() and np.isfinite(d[..., [0, 1, 2, 9, 10]]).all() and (c >= 0).all() and (c <= T * 83).all()
    for b in range(2):
        assert not d[b, c[b]:].any() and (d[b, :c[b], 9] > 0).all()
        assert ((d[b, :c[b], 10] >= 0) & (d[b, :c[b], 10] < sum(m.bbox_head.num_classes))).all()
    with pytest.raises(ValueError):
        m.forward(points[:, :4].contiguous(), offsets)
