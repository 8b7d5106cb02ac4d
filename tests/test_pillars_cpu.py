"""CPU: the point-cloud front end without a GPU -- the numpy statement of md_voxelize against the fixture the reference's own
points_to_voxel produced, the float64 statement of md_pillar_encode against a plain torch composition, the model build from the new
config, the reader's weight import / export, the argument checks of the two entry points (all before any device call) and the ISA audit
of csrc/pillars.hip."""
import ctypes as C
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from minddet_amd import _lib, det_ops, graphs, weights
from tests import pillar_contract as pc
from tests import abi_header as ah
from tests.abi_cases_points import CASES
from tests.abi_derive import attr, item, rc, refuse_single_defects, shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "pillar_vectors.npz")
CFG = os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc_points.py")
OLD_CFG = os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc.py")
OUT = ("_voxels", "_coors", "_num_points", "_voxel_num")


def fixture_case(z, name):
    src = "capped" if name == "uncapped" else name
    return (z[src + "_points"], z[src + "_offsets"], z[name + "_voxel_size"], z[name + "_range"], int(z[name + "_max_points"]),
            int(z[name + "_max_voxels"]))


# ------------------------------------------------------------------------------------------------------------------------ voxeliser
@pytest.mark.parametrize("name", ["capped", "uncapped", "f4"])
def test_voxeliser_statements_equal_the_reference_fixture(name):
    z = np.load(GOLD)
    args = fixture_case(z, name)
    for fn in (pc.voxelize_loop, pc.voxelize_ref):
        got = fn(*args)
        for g, k in zip(got, OUT):
            assert g.dtype == z[name + k].dtype and np.array_equal(g, z[name + k]), (fn.__name__, k)


def test_fixture_holds_the_plants():
    z = np.load(GOLD)
    pts, off, vs, rg, mp, mv = fixture_case(z, "capped")
    cell, valid = pc.cells_of(pts, vs, rg)
    assert (z["capped_voxel_num"] == mv).all() and (z["uncapped_voxel_num"] < int(z["uncapped_max_voxels"])).all()   # the cap bites / not
    assert (z["uncapped_voxel_num"] > mv).all()
    assert (z["capped_num_points"] == mp).any() and np.signbit(pts[:, :3]).any() and (pts[:, :3] == 0).any()
    for ax in range(3):                                      # outside in each axis and direction
        assert (pts[:, ax] < rg[ax]).any() and (pts[:, ax] >= rg[ax + 3]).any()
    assert (pts[:, 0] == rg[0]).any() and (pts[:, 0] == rg[3]).any()
    # a reciprocal multiply in place of the divide moves points of this cloud to other cells, and the result changes
    cell_r, _ = pc.cells_of(pts, vs, rg, reciprocal=True)
    assert (cell != cell_r).any()
    # the late dense cell: present uncapped with a full voxel, absent capped
    late = (3, int(np.floor((3.1 + 6.4) / 0.2)), int(np.floor((6.1 + 6.4) / 0.2)))   # (z, y, x) -- z = 0
    def rows(name):
        c = z[name + "_coors"][0]
        return np.nonzero((c[:, 2] == late[1]) & (c[:, 3] == late[2]) & (z[name + "_num_points"][0] > 0))[0]
    assert len(rows("capped")) == 0 and len(rows("uncapped")) == 1
    assert z["uncapped_num_points"][0, rows("uncapped")[0]] == mp


# ------------------------------------------------------------------------------------------------------------------- pillar encoder
def random_voxels(seed, B=2, MV=40, MP=6, F=5, hw=(16, 16)):
    """voxels as md_voxelize leaves them (zeros past num_points), counts 1, MP - 1 and MP among them, distinct cells"""
    rng = np.random.default_rng(seed)
    voxel_num = np.array([MV, MV // 2][:B] + [MV] * max(0, B - 2), np.int32)
    num = rng.integers(1, MP + 1, (B, MV)).astype(np.int32)
    num[:, 0], num[:, 1], num[:, 2] = 1, MP - 1, MP
    voxels = rng.normal(0, 2, (B, MV, MP, F)).astype(np.float32)
    voxels *= (np.arange(MP)[None, None, :, None] < num[..., None, None])
    coors = np.zeros((B, MV, 4), np.int32)
    for b in range(B):
        cell = rng.permutation(hw[0] * hw[1])[:MV]
        coors[b] = np.stack([np.full(MV, b), np.zeros(MV, np.int64), cell // hw[1], cell % hw[1]], 1)
    live = np.arange(MV)[None] < voxel_num[:, None]
    return voxels * live[..., None, None], num * live, coors * live[..., None], voxel_num


def random_pfn(seed, F=5, two=True, positive_shift=False):
    g = torch.Generator().manual_seed(seed)
    layers, cin = [], F + 5
    for units in ((32, 64) if two else (64,)):
        w = torch.randn((units, cin), generator=g) * (2.0 / cin) ** 0.5
        beta = torch.randn((units,), generator=g) * 0.5 + (0.8 if positive_shift else -0.3)
        bn = (torch.rand((units,), generator=g) + 0.5, beta, torch.randn((units,), generator=g) * 0.1,
              torch.rand((units,), generator=g) + 0.5, 1e-3)
        layers.append((w, bn))
        cin = 2 * units
    return layers


def torch_pfn(layers, voxels, num, coors, vx, vy, xo, yo, drop_padded=False):
    """PillarFeatureNet.construct (pillar_encoder.py:131-199) composed from plain torch ops in float64 on the FOLDED fp32 weights"""
    pk = det_ops.pack_pfn(layers)
    f = torch.from_numpy(voxels).double()
    V, MP, _ = f.shape
    n = torch.from_numpy(num).double().clamp(min=1).view(V, 1, 1)
    mean = f[:, :, :3].sum(1, keepdim=True) / n
    cx, cy = torch.from_numpy(coors[:, 3]).double().view(V, 1), torch.from_numpy(coors[:, 2]).double().view(V, 1)
    f32 = lambda v: float(np.float32(v))
    feats = torch.cat([f, f[:, :, :3] - mean, (f[:, :, 0] - (cx * f32(vx) + f32(xo))).unsqueeze(2),
                       (f[:, :, 1] - (cy * f32(vy) + f32(yo))).unsqueeze(2)], 2)
    mask = (torch.arange(MP).view(1, MP) < torch.from_numpy(num).view(V, 1))
    feats = feats * mask.unsqueeze(2)
    ws = [(pk.w1, pk.b1)] + ([(pk.w2, pk.b2)] if pk.w2 is not None else [])
    for i, (w, b) in enumerate(ws):
        x = torch.relu(torch.nn.functional.linear(feats, w.double(), b.double()))
        xm = (x.masked_fill(~mask.unsqueeze(2), float("-inf")) if drop_padded else x).max(1).values
        if i == len(ws) - 1:
            return xm.numpy()
        feats = torch.cat([x, xm.unsqueeze(1).expand(V, MP, xm.shape[1])], 2)


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("F", [4, 5])
def test_pfn_statement_equals_a_torch_composition(two, F):
    voxels, num, coors, voxel_num = random_voxels(3, F=F)
    layers = random_pfn(5, F=F, two=two, positive_shift=True)
    pk = det_ops.pack_pfn(layers)
    np_ = lambda t: None if t is None else t.numpy()
    at = (0.2, 0.2, -1.5, -1.5)
    feat, bound, live = pc.pfn_ref(voxels, num, coors, voxel_num, np_(pk.w1), np_(pk.b1), np_(pk.w2), np_(pk.b2), *at)
    B, MV = num.shape
    want = torch_pfn(layers, voxels.reshape(B * MV, *voxels.shape[2:]), num.reshape(-1), coors.reshape(-1, 4), *at).reshape(B, MV, 64)
    assert feat.shape == (B, MV, 64) and np.abs(feat - want)[live].max() < 1e-12
    assert (bound[live] > 0).all() and bound[live].max() < 1e-4 * max(1.0, np.abs(feat).max())
    # leaving the padded rows out of the maximum is a different function ON THIS DATA: both statements agree about that too
    dropped = torch_pfn(layers, voxels.reshape(B * MV, *voxels.shape[2:]), num.reshape(-1), coors.reshape(-1, 4), *at, drop_padded=True)
    dropped = dropped.reshape(B, MV, 64)
    skipped, _, _ = pc.pfn_ref(voxels, num, coors, voxel_num, np_(pk.w1), np_(pk.b1), np_(pk.w2), np_(pk.b2), *at, skip_padded=True)
    assert np.abs(skipped - dropped)[live].max() < 1e-12
    assert (np.abs(dropped - want)[live] > 100 * bound[live]).any()
    swapped, _, _ = pc.pfn_ref(voxels, num, coors, voxel_num, np_(pk.w1), np_(pk.b1), np_(pk.w2), np_(pk.b2), *at, swap_xy=True)
    assert (np.abs(swapped - want)[live] > 100 * bound[live]).any()


def test_bf16_interval():
    x = torch.randn(4096, dtype=torch.float64) * 3
    assert np.array_equal(pc.bf16_round(x.float().double().numpy()), x.float().bfloat16().double().numpy())
    lo, hi = pc.bf16_interval(np.array([1.00390625]), np.array([1e-7]))      # a midpoint of bf16 neighbours 1.0 and 1.0078125
    assert lo[0] == 1.0 and hi[0] == 1.0078125
    lo, hi = pc.bf16_interval(np.array([1.003]), np.array([1e-7]))
    assert lo[0] == hi[0] == 1.0


# ------------------------------------------------------------------------------------------------------------------------ the model
def _detector(seed=7, **over):
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(CFG)
    return build_detector(dict(dict(cfg.model), seed=seed, **over), cfg.train_cfg, cfg.test_cfg), cfg


def test_new_config_builds_the_pillar_detector_with_the_reference_values():
    from minddet.models import Config, build_detector
    from minddet_amd.registry import BACKBONES, DETECTORS, READERS

    m, cfg = _detector()
    assert type(m) is graphs.PillarDetector and type(m.detector) is graphs.PointPillars
    assert type(m.reader) is graphs.PillarFeatureNet and type(m.backbone) is graphs.PointPillarsScatter
    assert READERS.get("PillarFeatureNet") is graphs.PillarFeatureNet and BACKBONES.get("PointPillarsScatter") is graphs.PointPillarsScatter
    assert DETECTORS.get("PillarDetector") is graphs.PillarDetector and DETECTORS.get("PointPillars") is graphs.PointPillars
    r = cfg.model["reader"]
    assert list(r["num_filters"]) == [64, 64] and r["num_input_features"] == 5 and tuple(r["voxel_size"]) == (0.2, 0.2, 8)
    assert tuple(r["pc_range"]) == (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0) and not r["with_distance"]
    vg = cfg.model["voxel_generator"]
    assert vg["max_points_in_voxel"] == 20 and vg["max_voxel_num"] == 60000 and list(vg["voxel_size"]) == [0.2, 0.2, 8]
    assert m.grid_hw == (512, 512) and (m.max_points, m.max_voxels) == (20, 60000)
    assert [tuple(w.shape) for w, _ in m.reader.layers] == [(32, 10), (64, 64)] and all(bn[4] == 1e-3 for _, bn in m.reader.layers)
    assert np.float32(m.reader.x_offset) == np.float32(0.1 - 51.2) and m.reader.vx == 0.2
    assert m.neck is m.detector.neck and m.bbox_head.in_channels == 384
    old = Config.fromfile(OLD_CFG)
    assert type(build_detector(dict(old.model), old.train_cfg, old.test_cfg)) is graphs.PointPillars


def test_unsupported_reader_options_raise():
    base = dict(num_input_features=5, num_filters=[64, 64], voxel_size=(0.2, 0.2, 8), pc_range=(-51.2, -51.2, -5, 51.2, 51.2, 3))
    graphs.PillarFeatureNet(**base)
    graphs.PillarFeatureNet(**dict(base, num_filters=(64,), num_input_features=4))
    for bad in (dict(with_distance=True), dict(virtual=True), dict(num_filters=[32]), dict(num_filters=[64, 128]), dict(num_filters=[64, 64, 64]),
                dict(num_input_features=3), dict(num_input_features=6)):
        with pytest.raises(ValueError):
            graphs.PillarFeatureNet(**dict(base, **bad))
    with pytest.raises(ValueError):
        graphs.PointPillarsScatter(ds_factor=2)
    with pytest.raises(ValueError):
        graphs.PointPillarsScatter(num_input_features=32)
    with pytest.raises(ValueError):
        det_ops.pack_pfn([(torch.zeros((64, 11)), (torch.ones(64), torch.zeros(64), torch.zeros(64), torch.ones(64), 1e-3))])
    with pytest.raises(ValueError):
        _detector(voxel_generator=dict(range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], voxel_size=[0.2, 0.2, 4], max_points_in_voxel=20,
                                       max_voxel_num=100))


def test_pack_pfn_folds_the_batchnorm():
    layers = random_pfn(1)
    pk = det_ops.pack_pfn(layers)
    x = torch.randn((7, 10), generator=torch.Generator().manual_seed(2))
    w, (gamma, beta, mean, var, eps) = layers[0]
    want = (x.double() @ w.double().T - mean.double()) / torch.sqrt(var.double() + eps) * gamma.double() + beta.double()
    got = x.double() @ pk.w1.double().T + pk.b1.double()
    assert pk.w1.dtype == torch.float32 and tuple(pk.w2.shape) == (64, 64) and (got - want).abs().max() < 1e-5


def _same(a, b, naming):
    sa, sb = weights.reader_state(a, naming=naming), weights.reader_state(b, naming=naming)
    return sorted(sa) == sorted(sb) and all(np.array_equal(sa[k], sb[k]) for k in sa)


@pytest.mark.parametrize("naming", ["ms", "torch", "ms-custom-bn"])
def test_reader_weights_round_trip(naming):
    a, b = _detector(1)[0].reader, _detector(2)[0].reader
    base = "torch" if naming == "torch" else "ms"
    assert not _same(a, b, base)
    st = weights.reader_state(a, naming=base)
    assert len(st) == 2 * 5
    bn = ("gamma", "beta", "moving_mean", "moving_variance") if base == "ms" else ("weight", "bias", "running_mean", "running_var")
    assert {f"reader.pfn_layers.{i}.norm.{n}" for i in (0, 1) for n in bn} | {f"reader.pfn_layers.{i}.linear.weight" for i in (0, 1)} == set(st)
    assert st["reader.pfn_layers.0.linear.weight"].shape == (32, 10) and st["reader.pfn_layers.1.linear.weight"].shape == (64, 64)
    if naming == "torch":
        st = dict(st, **{"reader.pfn_layers.0.norm.num_batches_tracked": np.array(3)})
    if naming == "ms-custom-bn":      # the parameter names BatchNorm2dMasked registers
        st = {k.replace("moving_mean", "mean").replace("moving_variance", "variance"): v for k, v in st.items()}
        assert "reader.pfn_layers.1.norm.variance" in st
    assert weights.load_reader(b, st, naming="auto") == []
    assert _same(a, b, base)
    bad = dict(weights.reader_state(a))
    bad["reader.pfn_layers.1.linear.weight"] = np.zeros((64, 32), np.float32)
    with pytest.raises(ValueError):
        weights.load_reader(b, bad)
    del bad["reader.pfn_layers.1.linear.weight"]
    with pytest.raises(KeyError):
        weights.load_reader(b, bad)


# -------------------------------------------------------------------------------------------------------------------- ABI and ISA
def test_points_header_declares_the_two_symbols_and_the_main_header_none_of_them():
    pts = ah.header("minddet_hip_points.h")
    main = ah.header("minddet_hip.h")
    assert ah.aot_symbols(pts) == ["md_voxelize", "md_pillar_encode"] and '#include "minddet_hip.h"' in pts
    assert not {"md_voxelize", "md_pillar_encode"} & set(ah.aot_symbols(main))
    assert {c.sym for c in CASES} == {"md_voxelize", "md_pillar_encode"} and len({c.id for c in CASES}) == len(CASES)
    assert C.sizeof(det_ops._VoxelizeAttrs) == 4 * 11 and C.sizeof(det_ops._PillarEncodeAttrs) == 4 * 6
    assert "minddet_hip_points.h" in open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_points", case)


def test_attribute_and_shape_checks():
    from tests.abi_cases import F, T
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    vox, two, one = CASES
    ARG, SIZE = 2, 4

    for e in (attr("max_points", 5), attr("max_voxels", 7), item("voxel_size", 0, 0.0), item("voxel_size", 1, -0.2),
              item("voxel_size", 2, float("nan")), item("range", 0, 2.0), item("range", 5, float("inf")), shape(0, (16, 3)), shape(0, (16, 6)),
              shape(2, (3, 8, 4, 5)), shape(2, (2, 8, 4, 4)), shape(3, (2, 8, 3), "int32"), shape(4, (2, 9), "int32"), shape(5, (3,), "int32")):
        assert rc(vox, e) == ARG
    assert rc(vox, item("voxel_size", 0, 1e-7)) in (ARG, SIZE)                 # 32 million cells per row
    for case in (two, one):
        for e in (attr("with_distance", 1), attr("virtual_points", 1), attr("vx", float("nan")), shape(0, (2, 8, 4, 6)), shape(1, (2, 7), "int32"),
                  shape(2, (2, 8, 3), "int32"), shape(3, (1,), "int32"), shape(4, (48, 10)), shape(4, (case.operands[4].shape[0], 9)),
                  shape(5, (16,)), shape(8, (2, 16, 16, 32), "bfloat16"), shape(8, (3, 16, 16, 64), "bfloat16")):
            assert rc(case, e) == ARG, case.id
        assert rc(case, shape(0, (2, 8, 65, 5))) == SIZE                       # more rows than the kernel's slab
    assert rc(two, shape(6, (64, 32))) == ARG and rc(two, shape(7, (32,))) == ARG
    assert rc(two, shape(4, (64, 10))) == ARG and rc(one, shape(4, (32, 10))) == ARG      # the first layer's width follows the layer count

    def only_w2(c):
        c.operands[7] = T((64,), F, "opt", null=True)
    assert rc(two, only_w2) == ARG


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc + c++filt")
def test_pillars_kernels_pass_the_isa_audit():
    sys.path.insert(0, ROOT)
    from tools import isa_audit

    rows, bad = isa_audit.audit(files=("pillars.hip",))
    assert not bad, "\n".join(bad)                                   # no store-data hazard site
    txt = open(isa_audit.compile_isa(os.path.join(isa_audit.CSRC, "pillars.hip"))).read()
    meta = isa_audit._meta(txt)
    names = isa_audit.demangle(list(meta))
    kernels = {names[k]: v for k, v in meta.items()}
    enc = [d for d in kernels if "md::pillar_encode_kernel" in d]
    assert len(enc) == 4, sorted(kernels)                            # F = 4 / 5 x one / two layers
    assert sum("md::vox_" in d or "md::scan_" in d for d in kernels) == 9, sorted(kernels)
    for d, st in kernels.items():
        assert st["spill"] == 0 and st["sgpr_spill"] == 0 and st["scratch"] == 0, (d, st)
    assert all(kernels[d]["vgpr"] <= 256 for d in enc), {d: kernels[d]["vgpr"] for d in enc}   # two waves per SIMD stay resident
