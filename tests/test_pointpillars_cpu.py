"""CPU: the anchor-based PointPillars without a GPU -- the ABI of include/minddet_hip_pp.h (header, symbols, struct size, argument
checks before any device call), the three configs, the documented refusals, the block1 eps quirk, the float64 contract of
tests/pp_contract.py against the reference-generated vectors and its either-outcome cap, and the weight round trip."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from minddet_amd import _lib, det_ops, graphs, weights
from tests import pp_contract as ppc
from tests import abi_header as ah
from tests.abi_cases import I
from tests.abi_cases_pp import CASES
from tests.abi_derive import attr, rc, refuse_single_defects, shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = {n: os.path.join(ROOT, "configs", "pointpillars", f"pointpillars_{n}.py") for n in ("car_xyres16", "ped_cycle_xyres16", "tiny")}


def _detector(name, seed=7, **over):
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(CFG[name])
    return build_detector(dict(dict(cfg.model), seed=seed, **over), cfg.train_cfg, cfg.test_cfg), cfg


# ------------------------------------------------------------------------------------------------------------------------------ ABI
def test_pp_header_declares_the_two_symbols_and_the_main_header_neither():
    pp = ah.header("minddet_hip_pp.h")
    main = ah.header("minddet_hip.h")
    assert ah.aot_symbols(pp) == ["md_pp_scores", "md_pp_decode_selected"] and '#include "minddet_hip.h"' in pp
    assert not {"md_pp_scores", "md_pp_decode_selected"} & set(ah.aot_symbols(main))
    assert {c.sym for c in CASES} == {"md_pp_scores", "md_pp_decode_selected"} and len({c.id for c in CASES}) == len(CASES)
    fields = [re.fullmatch(r"int32_t\s+(\w+)", s).group(1) for s in ah.statements("md_pp_head_attrs", pp)]
    n_i32 = len(fields)
    assert n_i32 == 7 and C.sizeof(det_ops._PPHeadAttrs) == 4 * n_i32 == C.sizeof(CASES[0].extra)
    assert [f for f, _ in det_ops._PPHeadAttrs._fields_] == fields
    assert "minddet_hip_pp.h" in open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "md_pp_scores") and hasattr(lib, "md_pp_decode_selected")


def test_decode_and_standup_arithmetic_is_shared_by_both_translation_units():
    src = {n: open(os.path.join(ROOT, "minddet_amd", "csrc", n)).read() for n in ("detops.hip", "pphead.hip", "box_codec.h")}
    for n in ("detops.hip", "pphead.hip"):
        assert '#include "box_codec.h"' in src[n] and "second_box_decode_one(" in src[n] and "standup_one(" in src[n], n
    assert "sqrtf(" not in src["pphead.hip"] and "sinf(" not in src["pphead.hip"]      # no second statement of either formula
    assert "sqrtf(" in src["box_codec.h"] and "sinf(" in src["box_codec.h"]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_pp", case)


def test_semantic_refusals_return_2():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    sc, _, dec, dec9 = CASES
    ARG = 2

    for e in (attr("num_classes", 0), attr("num_classes", -1), attr("num_anchors", 0), attr("off_cls", -1), attr("off_cls", 21),
              attr("num_classes", 13), attr("score_mode", 1), shape(2, (1, 11)), shape(3, (1, 13), I), shape(2, (2, 12)),
              shape(1, (1, 11), "uint8")):
        assert rc(sc, e) == ARG
    for case in (dec, dec9):
        for e in (attr("self_train", 0), attr("num_anchors", 0), attr("off_box", -1), attr("off_box", 11), attr("off_dir", 21),
                  attr("off_dir", -2), shape(1, (11, 7)), shape(1, (13, 7)), shape(1, (12, 6)), shape(2, (1, 4), I), shape(2, (2, 5), I),
                  shape(3, (2,), I), shape(4, (1, 6)), shape(5, (1, 11), I), shape(6, (1, 4, 9)), shape(6, (1, 5, 8)), shape(7, (1, 6, 4)),
                  shape(8, (1, 4), I)):
            assert rc(case, e) == ARG, case.id
    assert rc(dec, shape(9, (1, 4, 7))) == ARG and rc(dec, shape(9, (1, 5, 9))) == ARG


# -------------------------------------------------------------------------------------------------------------------------- the model
def cfg_type(name):
    from minddet.models import Config

    return Config.fromfile(CFG[name]).model["type"]


def test_registry_takes_a_name_for_a_class():
    from minddet_amd.registry import Registry

    reg = Registry("thing")

    @reg.register_module
    class A:
        pass

    @reg.register_module(name="Other")
    class B:
        pass

    assert reg.get("A") is A and reg.get("Other") is B and reg.get("B") is None and len(reg) == 2
    with pytest.raises(KeyError):
        reg.register_module(A, name="Other")


def test_three_configs_build_with_the_reference_values():
    from minddet_amd.registry import DETECTORS

    # the class carries the reference's name; its registry key is its own, next to det3d's "PointPillars"
    assert DETECTORS.get("PointPillarsKITTI") is graphs.PointPillarsNet and DETECTORS.get("PointPillars") is graphs.PointPillars
    assert cfg_type("car_xyres16") == cfg_type("ped_cycle_xyres16") == cfg_type("tiny") == "PointPillarsKITTI"
    car, cfg = _detector("car_xyres16")
    assert type(car) is graphs.PointPillarsNet and isinstance(cfg.model, dict)
    assert car.grid_hw == (496, 432) and car.feature_hw == (248, 216) and car.num_anchors == 2 and car.num_class == 1
    assert car.bbox_head.head_channels == 20 and car.head_offsets() == dict(cls=0, box=2, dir_cls=16)
    assert car.feature_hw[0] * car.feature_hw[1] * car.num_anchors == 107136
    assert car.neck.out_channels == 384 and [len(b) for b in car.neck.blocks] == [4, 6, 6]
    assert [b[0].cout for b in car.neck.blocks] == [64, 128, 256] and [b[0].stride for b in car.neck.blocks] == [2, 2, 2]
    assert [type(d).__name__ for d in car.neck.deblocks] == ["ConvModule", "DeconvModule", "DeconvModule"]
    assert [(d.k, d.stride, d.cout) for d in car.neck.deblocks] == [(1, 1, 128), (2, 2, 128), (4, 4, 128)]
    assert (car.post.pre, car.post.post, car.post.score_thr, car.post.iou_thr) == (900, 300, 0.09, 0.01)
    assert car.anchor_area_threshold == 1 and car.pc_range == (0, -39.68, -3, 69.12, 39.68, 1) and car.voxel_size[:2] == (0.16, 0.16)
    g = car.generators[0]
    assert list(g._sizes) == [1.6, 3.9, 1.56] and list(g._anchor_strides) == [0.32, 0.32, 0.0] and list(g._rotations) == [0, 1.57]
    assert list(g._anchor_offsets) == [0.16, -39.52, -1.78]
    ped, _ = _detector("ped_cycle_xyres16")
    assert ped.grid_hw == (248, 296) and ped.feature_hw == (248, 296) and ped.num_anchors == 4 and ped.num_class == 2
    assert ped.bbox_head.head_channels == 44 and ped.head_offsets() == dict(cls=0, box=8, dir_cls=36)
    assert ped.feature_hw[0] * ped.feature_hw[1] * ped.num_anchors == 293632 and [b[0].stride for b in ped.neck.blocks] == [1, 2, 2]
    assert [list(g._sizes) for g in ped.generators] == [[0.6, 1.76, 1.73], [0.6, 0.8, 1.73]]
    tiny, _ = _detector("tiny")
    assert tiny.grid_hw == (32, 48) and tiny.feature_hw == (16, 24) and tiny.num_anchors == 4 and tiny.num_class == 2
    for m, want in ((car, 24), (ped, 48), (tiny, 48)):                    # the merged head tensor: channels rounded up to 8
        assert (m.bbox_head.head_channels + 7) // 8 * 8 == want
        assert [c.k for c in m.bbox_head.children()] == [1, 1, 1] and all(c.bn is None and c.bias is not None and c.act is None
                                                                          for c in m.bbox_head.children())


def test_block1_inner_batchnorms_use_the_default_eps():
    m, _ = _detector("car_xyres16")
    b1, b2, b3 = m.neck.blocks
    assert b1[0].bn[4] == 1e-3 and [c.bn[4] for c in b1[1:]] == [1e-5] * 3
    assert all(c.bn[4] == 1e-3 for c in b2 + b3 + m.neck.deblocks)
    # graphs.RPN without the argument is what it was: one eps everywhere, and the same random parameters
    a, b = graphs.RPN(seed=5), graphs.RPN(seed=5, inner_norm_eps=(1e-5, None, None))
    assert all(c.bn[4] == 1e-3 for c in a.children())
    assert all(torch.equal(x.weight if hasattr(x, "weight") else x.weight_t, y.weight if hasattr(y, "weight") else y.weight_t)
               for x, y in zip(a.children(), b.children()))


def test_unsupported_options_raise():
    for bad in (dict(voxel_feature_extractor=dict(num_filters=[64])), dict(middle_feature_extractor=dict()), dict(use_bev=True),
                dict(encode_background_as_zeros=False), dict(use_sigmoid_score=False), dict(use_self_train=False),
                dict(rpn=dict(layer_strides=[2, 2, 2], upsample_strides=[1, 2, 2]))):
        with pytest.raises(ValueError):
            _detector("tiny", **bad)
    from minddet.models import Config, build_detector
    cfg = Config.fromfile(CFG["tiny"])
    with pytest.raises(ValueError):
        build_detector(dict(cfg.model), None, None)
    with pytest.raises(ValueError):
        det_ops.PPHeadPost(dict(num_anchors=2, num_classes=1, off_cls=0, off_box=2, off_dir=16, nms_pre_max_size=9, nms_post_max_size=3,
                                nms_score_threshold=0.1, nms_iou_threshold=0.1, use_self_train=False))


def test_near_bbox_statement_equals_the_reference_vectors(golden):
    got = det_ops.rbbox2d_to_near_bbox(torch.from_numpy(golden["near_in"]))
    np.testing.assert_array_equal(got.numpy(), golden["near_out"])


# ----------------------------------------------------------------------------------------------------------------------- the contract
def test_contract_decode_and_standup_reproduce_the_reference_vectors(golden):
    """the float64 statements against the reference's own outputs: each within its own derived bound (far inside the 1e-5 the oracle
    test allows the standup boxes; the fp32 oracle reproduces codec_dec exactly, a float64 value can only lie within the bound)"""
    enc, anc = torch.from_numpy(golden["codec_enc"]).double(), torch.from_numpy(golden["codec_anchors"]).double()
    box = ppc.second_box_decode(enc, anc)
    err = (box.v - torch.from_numpy(golden["codec_dec"]).double()).abs()
    assert bool((err <= box.e).all()) and float(box.e.max()) < 2e-4 and float(err.max()) < 1e-5
    rb = torch.from_numpy(golden["near_in"]).double()
    st = ppc.standup(*(ppc.T(rb[:, j]) for j in range(5)))
    err = (st.v - torch.from_numpy(golden["standup_out"]).double()).abs()
    assert float(err.max()) <= 1e-5 and bool((err <= st.e + 1e-5).all()) and float(st.e.max()) < 1e-4


@pytest.mark.parametrize("name", ["clamp", "odd", "three"])
def test_generators_keep_the_either_outcome_share_under_the_cap(name):
    B, H, W, A, K, Cc = ppc.SHAPES[name]
    head, a, plants = ppc.make_head(name)
    mask = ppc.make_mask(name, all_masked_sample=0)
    out, n_dec, n_either = ppc.scores(head, mask, a)
    assert n_dec > 0 and n_either <= ppc.CAP * n_dec, (n_either, n_dec)
    cls = head[..., :A * K].float()
    assert -12.5 <= float(cls[cls < 20].min()) and float(cls[cls < 20].max()) <= 6.5
    N = H * W * A
    sc = torch.where(mask != 0, out["scores"].val.v, torch.full((B, N), -1.0, dtype=torch.float64)).float()
    # the reference's own values pass its own expectation; a label off by one class does not
    nb, worst, _ = ppc.check(sc, out["scores"])
    assert nb == 0 and worst <= 1.0
    want = torch.sigmoid(cls.double().reshape(B, N, K)).argmax(-1) if K > 1 else torch.zeros((B, N), dtype=torch.long)
    if K > 1:
        for b in range(B):
            assert n_either >= len(plants["saturated"][b])              # the saturated plants are the either-outcome set
            t = plants["ties"][b]
            lab = want.clone()
            lab[b, t] = 0
            assert bool(out["labels"](lab)[b, t].all())
            lab[b, t] = 1
            assert not bool(out["labels"](lab)[b, t].any())             # an exact tie goes to the lower class, nothing else passes
            s = plants["saturated"][b]
            for v in (0, 1):
                lab[b, s] = v
                assert bool(out["labels"](lab)[b, s].all())
    # decode: the device's top-k stands in as a plain sort here
    anchors = ppc.make_anchors(name)
    k = min(900, N)
    vals, idx = torch.sort(sc, dim=1, descending=True, stable=True)
    vals, idx = vals[:, :k].contiguous(), idx[:, :k].to(torch.int32).contiguous()
    cnt = (vals >= 0.09).sum(1).to(torch.int32)
    assert int(cnt[0]) == 0 and int(cnt[1]) > 0
    labels = torch.zeros((B, N), dtype=torch.int32)
    d, n_dec, n_either = ppc.decode_selected(head, anchors, idx, cnt, vals, labels, a)
    assert n_dec > 0 and n_either <= ppc.CAP * n_dec, (n_either, n_dec)
    rot = d["boxes"].val.v[..., 6][d["live"]]
    assert float((rot.abs() < 2.0 ** -7).double().mean()) < 0.01 and 0.2 < float((rot > 0).double().mean()) < 0.95
    assert bool(d["rot_fixed"].any()) and bool((d["live"] & ~d["rot_fixed"]).any()) and bool((d["dir_labels"] == 1).any())
    assert float(d["boxes"].val.e.max()) < 1e-4 and float(d["standup"].val.e.max()) < 1e-4
    assert not bool(d["boxes"].val.v[~d["live"]].any())


# ------------------------------------------------------------------------------------------------------------------------- weights
def _same(a, b, naming):
    sa, sb = weights.pointpillars_state(a, naming=naming), weights.pointpillars_state(b, naming=naming)
    return sorted(sa) == sorted(sb) and all(sa[k].dtype == sb[k].dtype and np.array_equal(sa[k], sb[k]) for k in sa)


@pytest.mark.parametrize("naming", ["ms", "torch", "ms-training-prefix"])
def test_weights_round_trip(naming):
    a, b = _detector("tiny", 1)[0], _detector("tiny", 2)[0]
    base = "torch" if naming == "torch" else "ms"
    assert not _same(a, b, base)
    st = weights.pointpillars_state(a, naming=base)
    bn = ("gamma", "beta", "moving_mean", "moving_variance") if base == "ms" else ("weight", "bias", "running_mean", "running_var")
    want = {f"rpn.block{i}.{3 * j}.weight" for i, n in ((1, 2), (2, 3), (3, 2)) for j in range(n)}
    want |= {f"rpn.block{i}.{3 * j + 1}.{s}" for i, n in ((1, 2), (2, 3), (3, 2)) for j in range(n) for s in bn}
    want |= {f"rpn.deconv{i}.0.weight" for i in (1, 2, 3)} | {f"rpn.deconv{i}.1.{s}" for i in (1, 2, 3) for s in bn}
    want |= {f"rpn.{h}.{s}" for h in ("conv_cls", "conv_box", "conv_dir_cls") for s in ("weight", "bias")}
    assert set(st) == want
    # Conv2dTranspose layout [Cin, Cout, k, k] for every deblock, the 1x1 one included
    assert st["rpn.deconv1.0.weight"].shape == (16, 16, 1, 1) and st["rpn.deconv3.0.weight"].shape == (32, 16, 4, 4)
    assert st["rpn.conv_box.weight"].shape == (28, 48, 1, 1) and st["rpn.conv_cls.bias"].shape == (8,)
    assert np.array_equal(st["rpn.deconv1.0.weight"][:, :, 0, 0], a.neck.deblocks[0].weight[:, :, 0, 0].numpy().T)
    if naming == "torch":
        st = dict(st, **{"rpn.block1.1.num_batches_tracked": np.array(3)})
    if naming == "ms-training-prefix":
        st = {"network.network." + k: v for k, v in st.items()}
    assert weights.load_pointpillars(b, st, naming="auto") == []
    assert _same(a, b, base)
    bad = dict(weights.pointpillars_state(a))
    bad["rpn.conv_box.weight"] = np.zeros((28, 32, 1, 1), np.float32)
    with pytest.raises(ValueError):
        weights.load_pointpillars(b, bad)
    del bad["rpn.conv_box.weight"]
    with pytest.raises(KeyError):
        weights.load_pointpillars(b, bad)
