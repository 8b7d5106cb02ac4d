"""CPU: the KITTI PointPillars front end without a GPU -- the ABI of include/minddet_hip_ppreader.h (header, symbols, struct sizes,
argument checks before any device call), the interval contract of tests/pp_reader_contract.py against an independent per-voxel loop
and against six devices the header excludes, the three `_points` configs, the unchanged old configs and refusals, and the weight
round trip."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from minddet_amd import _lib, det_ops, graphs, weights
from tests import pp_reader_contract as prc
from tests import abi_header as ah
from tests.abi_cases import I
from tests.abi_cases_ppreader import CASES
from tests.abi_derive import attr, rc, refuse_single_defects, shape
from tests.pillar_contract import bf16_round

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("car_xyres16", "ped_cycle_xyres16", "tiny")
CFG = {n + s: os.path.join(ROOT, "configs", "pointpillars", f"pointpillars_{n}{s}.py") for n in NAMES for s in ("", "_points")}
CAP = 0.01          # share of outputs on which the contract admits two bf16 values
VS, PCR = (0.16, 0.16, 4.0), (0, -39.68, -3, 69.12, 39.68, 1)
OFF = tuple(v / 2 + lo for v, lo in zip(VS, PCR[:3]))
SYMS = ["md_pp_pillar_encode", "md_pp_anchor_mask"]


def _detector(name, seed=7, **over):
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(CFG[name])
    return build_detector(dict(dict(cfg.model), seed=seed, **over), cfg.train_cfg, cfg.test_cfg), cfg


# ------------------------------------------------------------------------------------------------------------------------------ ABI
def test_ppreader_header_declares_the_two_symbols_and_no_other_header_does():
    hdr = ah.header("minddet_hip_ppreader.h")
    assert ah.aot_symbols(hdr) == SYMS and '#include "minddet_hip.h"' in hdr
    for other in ("minddet_hip.h", "minddet_hip_points.h", "minddet_hip_pp.h", "minddet_hip_chain.h"):
        assert not set(SYMS) & set(ah.aot_symbols(ah.header(other))), other
    assert {c.sym for c in CASES} == set(SYMS) and len({c.id for c in CASES}) == len(CASES)
    body = ah.statements("md_pp_pillar_encode_attrs", hdr)
    names = [n.strip() for s in body for n in re.fullmatch(r"(?:float|int32_t)\s+(.+)", s).group(1).split(",")]
    assert names == [f for f, _ in det_ops._PPPillarEncodeAttrs._fields_]
    assert C.sizeof(det_ops._PPPillarEncodeAttrs) == 4 * 8 == C.sizeof(CASES[0].extra)
    assert C.sizeof(det_ops._AnchorMaskAttrs) == 4 * 7 == C.sizeof(CASES[2].extra)
    assert "minddet_hip_ppreader.h" in open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    assert "pointpillars.py:" in hdr and "preprocess.py:211-225" in hdr and "box_np_ops.py:745-776" in hdr      # every entry cites its lines
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, s) for s in SYMS)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_ppreader", case)


def test_documented_refusals():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    k10, k11, area, plain = CASES
    ARG, SIZE = 2, 4

    for case in (k10, k11):
        for e in (attr("reserved0", 1), attr("with_distance", 1 - case.extra.with_distance), attr("with_distance", 2), attr("vx", 0.0),
                  attr("vy", -0.16), attr("vz", float("nan")), attr("vx", float("inf")), attr("x_offset", float("nan")),
                  attr("z_offset", float("inf")), shape(0, (2, 8, 6, 5)), shape(0, (2, 8, 6, 3)), shape(0, (3, 8, 6, 4)), shape(1, (2, 7), I),
                  shape(2, (2, 8, 3), I), shape(3, (1,), I), shape(4, (64, 9)), shape(4, (64, 12)), shape(4, (32, 10 + case.extra.with_distance)),
                  shape(5, (32,)), shape(6, (63,)), shape(7, (2, 16, 16, 32), "bfloat16"), shape(7, (3, 16, 16, 64), "bfloat16")):
            assert rc(case, e) == ARG, case.id
        assert rc(case, shape(0, (2, 8, 33, 4))) == SIZE                          # more rows than the 32 of the MFMA tile
        assert rc(case, shape(7, (2, 70000, 16, 64), "bfloat16")) == SIZE
    for case in (area, plain):
        for e in (shape(0, (2, 8, 3), I), shape(0, (3, 8, 4), I), shape(1, (3,), I), shape(2, (5, 5)), shape(3, (2, 6), "uint8"),
                  shape(3, (1, 5), "uint8")):
            assert rc(case, e) == ARG, case.id
        assert rc(case, attr("grid_x", 0)) == SIZE and rc(case, attr("grid_y", -3)) == SIZE and rc(case, attr("grid_x", 1 << 30)) == SIZE
    assert rc(area, shape(4, (2, 6))) == ARG and rc(area, shape(4, (3, 5))) == ARG


# ----------------------------------------------------------------------------------------------------------------------- the contract
_shared = {}


def shared_case():
    """B = 2, MV = 1200, MP = 32 on the Car grid, weights N(0, 2 / K): made once, never modified"""
    if not _shared:
        v, n, c, vn = prc.car_like_voxels(1, B=2, MV=1200, MP=32, voxel_size=VS, pc_range=PCR)
        w, sc, sh = prc.random_reader(2)
        lo, hi, live = prc.interval(v, n, c, vn, w, sc, sh, VS, OFF)
        for a in (v, n, c, vn, w, sc, sh, lo, hi, live):
            a.setflags(write=False)
        _shared.update(v=v, n=n, c=c, vn=vn, w=w, sc=sc, sh=sh, lo=lo, hi=hi, live=live)
    return _shared


def test_generator_holds_the_plants_and_stays_under_the_cap():
    s = shared_case()
    assert {0, 1, 31, 32} <= set(s["n"][0][s["live"][0]].tolist()) and s["vn"].tolist() == [1200, 600]
    assert (s["n"][~s["live"]] > 32).any() and (s["n"][~s["live"]] < 0).any()                   # garbage past voxel_num
    assert (s["sh"] > 0).any() and (s["sh"] < 0).any() and (s["sc"] < 0).any() and (s["sc"] > 0).any()
    either = (s["lo"] != s["hi"])[s["live"]].mean()
    print(f"either-outcome share {either:.5f} of {int(s['live'].sum()) * 64} outputs")
    assert 0 < either < CAP and (s["lo"] <= s["hi"]).all() and (s["lo"] >= 0).all()
    # padded rows win some maxima: a voxel with one point gives relu(fp16(shift)) where that is the largest
    pad = bf16_round(np.maximum(s["sh"].astype(np.float16).astype(np.float64), 0))
    one = s["live"] & (s["n"] == 1)
    assert (s["lo"][one] == pad).any() and (s["hi"][one] > pad).any()
    assert (s["lo"][0, 3] == pad).all() and (s["hi"][0, 3] == pad).all()                         # the live row without points


@pytest.mark.parametrize("with_distance", [False, True])
def test_contract_against_an_independent_per_voxel_loop(with_distance):
    """every value written out voxel by voxel with scalar-style operations: float32 features in the header's order, fp16 casts, the dot
    product in float64 (exact), the affine in float64 rounded once to fp32 (the FMA form), fp16, ReLU, maximum, bf16 through torch"""
    v, n, c, vn = prc.car_like_voxels(5, B=2, MV=90, MP=32, voxel_size=VS, pc_range=PCR)
    w, sc, sh = prc.random_reader(6, K=10 + with_distance)
    lo, hi, live = prc.interval(v, n, c, vn, w, sc, sh, VS, OFF, with_distance)
    f32, f16 = np.float32, np.float16
    w16 = w.astype(f16).astype(np.float64)
    seen = 0
    for b in range(2):
        for i in range(int(vn[b])):
            k = min(max(int(n[b, i]), 0), 32)
            p = v[b, i]
            s = np.zeros(3, f32)
            for r in range(k):
                s = s + p[r, :3]
            mean = s / f32(max(k, 1))
            ctr = np.array([f32(c[b, i, 3]) * f32(VS[0]) + f32(OFF[0]), f32(c[b, i, 2]) * f32(VS[1]) + f32(OFF[1]),
                            f32(c[b, i, 1]) * f32(VS[2]) + f32(OFF[2])], f32)
            rows = np.zeros((32, 10 + with_distance), f32)
            for r in range(k):
                feat = [p[r, 0], p[r, 1], p[r, 2], p[r, 3], *(p[r, :3] - mean), *(p[r, :3] - ctr)]
                if with_distance:
                    feat.append(np.sqrt((p[r, 0] * p[r, 0] + p[r, 1] * p[r, 1]) + p[r, 2] * p[r, 2]))
                rows[r] = feat
            d = (rows.astype(f16).astype(np.float64) @ w16.T).astype(f16).astype(np.float64)
            y = (sc.astype(np.float64) * d + sh.astype(np.float64)).astype(f32).astype(f16).astype(f32)
            m = torch.from_numpy(np.maximum(y, 0).max(0)).to(torch.bfloat16).double().numpy()
            assert ((m >= lo[b, i]) & (m <= hi[b, i])).all(), (b, i, k)
            seen += 1
    assert seen == int(vn.sum()) and live.sum() == vn.sum()


def test_an_admissible_device_passes_and_each_excluded_one_is_seen():
    s = shared_case()
    args = (s["v"], s["n"], s["c"], s["w"], s["sc"], s["sh"], VS, OFF)
    outside = lambda g: float(((g < s["lo"]) | (g > s["hi"]))[s["live"]].mean())
    assert outside(prc.emulate(*args)) == 0.0
    shares = {wrong: outside(prc.emulate(*args, wrong=wrong)) for wrong in prc.WRONG}
    print({k: round(v, 4) for k, v in shares.items()})
    assert all(v > CAP for v in shares.values()), shares            # each leaves the interval on more outputs than the contract is open on
    assert shares["no_z_centre"] > 0.3


def test_interval_is_open_exactly_where_a_rounding_midpoint_is_near():
    """a single channel, a single point: d = fp16(1 * x) and y = fp16(d + shift) with the sum on an fp16 midpoint"""
    v = np.zeros((1, 1, 32, 4), np.float32)
    v[0, 0, 0] = (3.0, 0, 0, 0)
    n, c, vn = np.array([[1]], np.int32), np.zeros((1, 1, 4), np.int32), np.array([1], np.int32)
    w = np.zeros((64, 10), np.float32)
    w[:, 0] = 1.0
    sc, sh = np.ones(64, np.float32), np.zeros(64, np.float32)
    sh[1] = 2.0 ** -7 + 2.0 ** -10      # 3 + 2^-7 + 2^-10: halfway between two fp16 values, 3 + 2^-7 (a bf16 tie, to 3) and 3 + 2^-7 + 2^-9
    lo, hi, _ = prc.interval(v, n, c, vn, w, sc, sh, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    assert lo[0, 0, 0] == hi[0, 0, 0] == 3.0
    assert lo[0, 0, 1] == 3.0 and hi[0, 0, 1] == 3.015625             # either fp16 neighbour is admissible, and bf16 tells them apart


# ------------------------------------------------------------------------------------------------------------------------ the model
def test_new_configs_build_the_points_detector_with_the_reference_values():
    from minddet_amd.registry import DETECTORS, READERS

    assert DETECTORS.get("PointPillarsKITTIPoints") is graphs.PointPillarsKITTIPoints and READERS.get("PPPillarFeatureNet") is graphs.PPPillarFeatureNet
    want = dict(car_xyres16=((496, 432), (248, 216), 2, 107136, 32, 40000), ped_cycle_xyres16=((248, 296), (248, 296), 4, 293632, 32, 40000),
                tiny=((32, 48), (16, 24), 4, 1536, 8, 256))
    for name, (grid, feat, A, N, mp, mv) in want.items():
        m, cfg = _detector(name + "_points")
        old, old_cfg = _detector(name)
        assert type(m) is graphs.PointPillarsKITTIPoints and type(m.inner) is graphs.PointPillarsNet and type(old) is graphs.PointPillarsNet
        assert m.grid_hw == grid and m.inner.feature_hw == feat and m.inner.num_anchors == A and feat[0] * feat[1] * A == N
        assert (m.max_points, m.max_voxels) == (mp, mv)
        vfe = cfg.model["voxel_feature_extractor"]
        assert list(vfe["num_filters"]) == [64] and vfe["with_distance"] is False and cfg.model["num_point_features"] == 4
        assert cfg.model["middle_feature_extractor"] is None and cfg.model["use_norm"] is True
        r = m.reader
        assert type(r) is graphs.PPPillarFeatureNet and [tuple(w.shape) for w, _ in r.layers] == [(64, 10)] and r.layers[0][1][4] == 1e-3
        vs, pr = cfg.model["voxel_generator"]["voxel_size"], cfg.model["voxel_generator"]["point_cloud_range"]
        assert r.voxel_size == tuple(vs) and r.offsets == tuple(v / 2 + lo for v, lo in zip(vs, pr[:3]))
        # everything behind the front end is the old config's model: same options, same weights at the same seed
        rest = {k: v for k, v in cfg.model.items() if k not in ("type", "voxel_feature_extractor", "middle_feature_extractor",
                                                                "num_point_features", "use_norm")}
        assert rest == {k: v for k, v in old_cfg.model.items() if k != "type"} and cfg.test_cfg == old_cfg.test_cfg
        sa, sb = weights.pointpillars_state(m.inner), weights.pointpillars_state(old)
        assert sorted(sa) == sorted(sb) and all(np.array_equal(sa[k], sb[k]) for k in sa)
        assert m.neck is m.inner.neck and m.bbox_head is m.inner.bbox_head
    assert graphs.PPPillarFeatureNet(with_distance=True).layers[0][0].shape == (64, 11)


def test_old_configs_and_refusals_are_unchanged():
    from minddet.models import Config

    for name in NAMES:
        assert Config.fromfile(CFG[name]).model["type"] == "PointPillarsKITTI"
    for bad in (dict(voxel_feature_extractor=dict(num_filters=[64])), dict(middle_feature_extractor=dict())):
        with pytest.raises(ValueError, match="PointPillarsKITTIPoints"):
            _detector("tiny", **bad)
    # the new type's own refusals, and the inner model's passed on
    for bad in (dict(voxel_feature_extractor=dict(num_filters=[64, 64])), dict(voxel_feature_extractor=dict(num_filters=[32])),
                dict(use_norm=False), dict(num_point_features=5), dict(num_point_features=3), dict(middle_feature_extractor=dict(ds_factor=2)),
                dict(voxel_feature_extractor=dict(num_filters=[64], virtual=True)), dict(use_bev=True), dict(use_self_train=False),
                dict(voxel_generator=dict(point_cloud_range=[0, -2.56, -2.5, 7.68, 2.56, 0.5], voxel_size=[0.16, 0.16, 3],
                                          max_number_of_points_per_voxel=33, max_number_of_voxels=256)),
                dict(voxel_generator=dict(point_cloud_range=[0, -2.56, -2.5, 7.68, 2.56, 0.5], voxel_size=[0.16, 0.16, 1.5],
                                          max_number_of_points_per_voxel=8, max_number_of_voxels=256))):
        with pytest.raises(ValueError):
            _detector("tiny_points", **bad)
    for bad in (dict(use_norm=False), dict(num_filters=(64, 64)), dict(num_filters=(32,)), dict(num_input_features=5)):
        with pytest.raises(ValueError):
            graphs.PPPillarFeatureNet(**bad)
    one = (torch.ones(64), torch.zeros(64), torch.zeros(64), torch.ones(64), 1e-3)
    for bad in ([(torch.zeros((64, 9)), one)], [(torch.zeros((32, 10)), one)], [(torch.zeros((64, 10)), one)] * 2):
        with pytest.raises(ValueError):
            det_ops.pack_pp_pfn(bad)


def test_pack_keeps_the_raw_weight_and_folds_the_batchnorm_in_fp32():
    r = graphs.PPPillarFeatureNet(seed=3)
    w, (gamma, beta, mean, var, eps) = r.layers[0]
    pk = det_ops.pack_pp_pfn(r.layers)
    assert pk.w.dtype == torch.float32 and torch.equal(pk.w, w) and (gamma != 1).any() and (beta > 0).any() and (beta < 0).any()
    scale = gamma / torch.sqrt(var + np.float32(eps))
    assert torch.equal(pk.scale, scale) and torch.equal(pk.shift, beta - mean * scale)
    x = torch.randn((5, 64), generator=torch.Generator().manual_seed(1)).double()
    want = (x - mean.double()) / torch.sqrt(var.double() + eps) * gamma.double() + beta.double()
    assert (x * pk.scale.double() + pk.shift.double() - want).abs().max() < 1e-5


def _same(a, b, naming):
    sa, sb = weights.pointpillars_points_state(a, naming=naming), weights.pointpillars_points_state(b, naming=naming)
    return sorted(sa) == sorted(sb) and all(sa[k].dtype == sb[k].dtype and np.array_equal(sa[k], sb[k]) for k in sa)


@pytest.mark.parametrize("naming", ["ms", "torch", "ms-training-prefix"])
def test_weights_round_trip(naming):
    a, b = _detector("tiny_points", 1)[0], _detector("tiny_points", 2)[0]
    base = "torch" if naming == "torch" else "ms"
    assert not _same(a, b, base)
    st = weights.pointpillars_points_state(a, naming=base)
    bn = ("gamma", "beta", "moving_mean", "moving_variance") if base == "ms" else ("weight", "bias", "running_mean", "running_var")
    reader_keys = {"voxel_feature_extractor.pfn_layers.0.linear.weight"} | {f"voxel_feature_extractor.pfn_layers.0.norm.{n}" for n in bn}
    assert reader_keys <= set(st) and set(st) - reader_keys == set(weights.pointpillars_state(a.inner, naming=base))
    assert st["voxel_feature_extractor.pfn_layers.0.linear.weight"].shape == (64, 10)
    if naming == "torch":
        st = dict(st, **{"voxel_feature_extractor.pfn_layers.0.norm.num_batches_tracked": np.array(3)})
    if naming == "ms-training-prefix":
        st = {"network.network." + k: v for k, v in st.items()}
    assert weights.load_pointpillars_points(b, st, naming="auto") == []
    assert _same(a, b, base)
    assert torch.equal(a.reader.layers[0][0], b.reader.layers[0][0]) and torch.equal(a.reader.layers[0][1][1], b.reader.layers[0][1][1])
    bad = dict(weights.pointpillars_points_state(a))
    bad["voxel_feature_extractor.pfn_layers.0.linear.weight"] = np.zeros((64, 9), np.float32)
    with pytest.raises(ValueError):
        weights.load_pointpillars_points(b, bad)
    del bad["voxel_feature_extractor.pfn_layers.0.linear.weight"]
    with pytest.raises(KeyError):
        weights.load_pointpillars_points(b, bad)
    assert weights.load_pointpillars_points(b, dict(weights.pointpillars_points_state(a), extra_key=np.zeros(1))) == ["extra_key"]
