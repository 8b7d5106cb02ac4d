"""CPU: the CenterNet training targets without a GPU -- the ABI of include/minddet_hip_cn.h (the function exported,
the semantic refusals answered before any device call, the ctypes mirrors laid out as the header says), the contract
tests/cn_targets_contract.py against the reference's own outputs (tests/golden/cn_target_vectors.npz, written by
tests/golden/gen_cn_targets.py from COCOHP.preprocess_fn), the flip and affine transform in front of it, and the configs."""
import ctypes as C
import os

import numpy as np
import pytest

from minddet_amd import det_ops
from tests import cn_targets_contract as ct
from tests import abi_header as ah
from tests.abi_cases import I, U8
from tests.abi_cases_cn import CASES, TARGET_CASES, CNLoss, CNTargets
from tests.abi_derive import attr, both, lib_handle, rc, refuse_single_defects, shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = ah.header("minddet_hip_cn.h")
GOLD = os.path.join(ROOT, "tests", "golden", "cn_target_vectors.npz")
NAMES = ("small", "tiles", "plants")


def fixture_case(name):
    """-> (dict of the recorded inputs: bboxes, category_id, num_objects, trans_output, flip_width, post_boxes, post_classes; keyword
    arguments of the contract / of det_ops.cn_assign_targets; the reference's outputs)"""
    z = np.load(GOLD)
    C_, H, W, M = (int(v) for v in z[name + "_meta"])
    kw = dict(num_classes=C_, feature_map_size=(W, H), max_objs=M, min_overlap=float(z["min_overlap"]))
    inputs = {k: z[name + "_" + k] for k in ("bboxes", "category_id", "num_objects", "trans_output", "flip_width", "post_boxes", "post_classes")}
    return inputs, kw, {k: z[name + "_" + k] for k in ct.KEYS}


def test_header_declares_the_three_symbols_and_the_library_exports_them():
    assert ah.aot_symbols(HDR) == ["md_cn_assign_targets", "md_cn_loss", "md_cn_loss_grad"] and '#include "minddet_hip.h"' in HDR
    assert "dataset.py:317-384" in HDR and "image.py:94-144" in HDR and "centernet_det.py:177-237" in HDR and "utils.py:48-245" in HDR
    assert "minddet_hip_cn.h" in open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    assert {c.sym for c in CASES} == {"md_cn_assign_targets", "md_cn_loss", "md_cn_loss_grad"} and len({c.id for c in CASES}) == len(CASES)
    lib = lib_handle()
    for sym in ("md_cn_assign_targets", "md_cn_loss", "md_cn_loss_grad"):
        assert getattr(lib, sym)(0, None, None, None, None, None, None) == 1             # wrong parameter count, before anything else


def test_ctypes_mirrors_have_the_headers_layout():
    for name, mirrors, size in (("md_cn_targets_attrs", (det_ops._CNTargetsAttrs, CNTargets), 4),
                                ("md_cn_loss_attrs", (det_ops._CNLossAttrs, CNLoss), 28)):
        want = ah.struct_of(name, HDR)
        assert C.sizeof(want) == size
        for got in mirrors:
            assert C.sizeof(got) == size and ah.layout(got) == ah.layout(want), got
    src = "".join(open(os.path.join(ROOT, "minddet_amd", "csrc", f)).read() for f in ("cntargets.hip", "cnloss.hip"))
    assert "static_assert(sizeof(md_cn_targets_attrs) == 4" in src and "static_assert(sizeof(md_cn_loss_attrs) == 4 * 4 + 3 * 4" in src
    defines = ah.defines(HDR)
    assert (defines["MD_CN_MAX_OBJS"], defines["MD_CN_LOSS_STRIP"], defines["MD_CN_LOSS_COUNT_CHUNK"]) == (det_ops.CN_MAX_OBJS, 64, 16384)
    # (each decides the library's answer: 64 cells are one strip of 16 bytes, 16384 heat-map elements one count of 4)
    assert [det_ops.cn_loss_workspace_bytes(1, 1, 1, w) for w in (64, 65)] == [8 * (4 + 2) + 4, 8 * (4 + 4) + 4]
    assert [det_ops.cn_loss_workspace_bytes(1, c, 128, 128) for c in (1, 2)] == [8 * (4 + 512) + 4, 8 * (4 + 512) + 8]


@pytest.mark.parametrize("case", TARGET_CASES, ids=[c.id for c in TARGET_CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_cn", case)


def test_semantic_refusals_return_the_documented_codes():
    ARG, SIZE = 2, 4
    case = TARGET_CASES[0]
    nan, inf = float("nan"), float("inf")
    edits = [
        both(shape(0, (1, 5, 4)), shape(1, (1, 5), I)),                                   # G > M
        attr("min_overlap", nan), attr("min_overlap", 0.0), attr("min_overlap", 1.0), attr("min_overlap", -0.1), attr("min_overlap", inf),
        shape(0, (1, 3, 5)), shape(0, (2, 3, 4)), shape(1, (1, 4), I), shape(2, (2, 3, 8, 12)), shape(2, (1, 3, 0, 12)),
        shape(3, (1, 5), I), shape(3, (2, 4), I), shape(4, (1, 3), U8), shape(5, (1, 4, 3)), shape(5, (1, 5, 2)), shape(6, (2, 4, 2)),
        shape(6, (1, 4, 1)),
    ]
    for i, e in enumerate(edits):
        assert rc(case, e) == ARG, i
    big = 1100                                                                            # M above the LDS bound
    grow = both(shape(3, (1, big), I), shape(4, (1, big), U8), shape(5, (1, big, 2)), shape(6, (1, big, 2)))
    assert rc(case, grow) == SIZE
    assert rc(case, shape(2, (1, 70000, 8, 12))) == SIZE                               # C above the grid bound
    assert rc(case, shape(2, (1, 3, 1 << 15, 1 << 14))) == SIZE                        # an operand of 2^30 elements and more
    assert rc(TARGET_CASES[1], shape(7, (63,), U8)) == SIZE                            # one byte short of 16 B M
    for ok in (1e-9, 0.999, float(np.float32(1.0) - np.float32(2.0) ** -24)):             # every fp32 value inside (0, 1) passes the checks
        assert rc(case, both(attr("min_overlap", ok), shape(2, (1, 70000, 8, 12)))) == SIZE


@pytest.mark.parametrize("name", NAMES)
def test_contract_equals_the_reference(name):
    inp, kw, want = fixture_case(name)
    got = ct.assign(inp["post_boxes"], inp["post_classes"], **kw)
    for k in ("ind", "reg_mask"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    for k in ("hm", "wh", "reg"):                                                         # bit for bit
        assert got[k].shape == want[k].shape and np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), k


@pytest.mark.parametrize("name", NAMES)
def test_flip_and_affine_transform_give_the_recorded_boxes(name):
    """the steps of det_ops.CenterNetTargets in front of the operator, in numpy: bit-equal to what the reference's affine_transform
    returned, on the rows the reference processed (the first max_objs of num_objects)"""
    inp, kw, _ = fixture_case(name)
    M = kw["max_objs"]
    post = ct.post_affine(inp["bboxes"][:, :M], inp["trans_output"], inp["flip_width"])
    for b, n in enumerate(inp["num_objects"]):
        n = min(int(n), M)
        nan_row = np.isnan(inp["post_boxes"][b, :n]).any(1)        # (a NaN x makes 0 * x + 1 * y a NaN too: the row stays a NaN row)
        assert np.array_equal(np.isnan(post[b, :n]).any(1), nan_row)
        assert np.array_equal(post[b, :n][~nan_row].view(np.int32), inp["post_boxes"][b, :n][~nan_row].view(np.int32)), b
    assert ct.overlap_of(0.7) == float(np.float32(0.7)) != 0.7 and ct.overlap_of(0.5) == 0.5


def test_fixture_carries_what_the_cases_promise():
    z = np.load(GOLD)
    assert int(str(z["numpy_version"]).split(".")[0]) >= 2 and os.path.getsize(GOLD) < 300 * 1024
    inp, kw, want = fixture_case("small")
    assert want["hm"].shape == (2, 5, 24, 40) and kw["max_objs"] == 32 and inp["num_objects"].tolist() == [40, 14]
    assert inp["flip_width"][0] > 0 and inp["flip_width"][1] == 0 and inp["bboxes"].shape == (2, 40, 4) and inp["post_boxes"].shape == (2, 32, 4)
    assert want["reg_mask"][0].sum() > 8 and want["reg_mask"][1].sum() > 8
    m0 = want["reg_mask"][0]
    assert (m0[:-1] == 0).any() and m0[np.flatnonzero(m0 == 0)[0]:].any()                 # a zero slot between used ones
    inp, kw, want = fixture_case("tiles")
    assert want["hm"].shape == (1, 3, 40, 72)
    hm = want["hm"][0].max(0)
    pb = inp["post_boxes"][0]
    assert ((pb[:, 0] < 0) & (pb[:, 1] < 0)).any() and ((pb[:, 2] > 71) & (pb[:, 1] < 0)).any() and ((pb[:, 0] < 0) & (pb[:, 3] > 39)).any() \
        and ((pb[:, 2] > 71) & (pb[:, 3] > 39)).any()                                     # boxes over the four corners, cut by the clip
    assert ((hm[:, 63] > 0) & (hm[:, 64] > 0)).any() and want["reg_mask"][0, :16].sum() >= 14
    assert ((hm[15] > 0) & (hm[16] > 0)).any() and ((hm[31] > 0) & (hm[32] > 0)).any()
    inp, kw, want = fixture_case("plants")
    assert want["hm"].shape == (1, 3, 16, 16) and np.array_equal(inp["trans_output"][0], [[1, 0, 0], [0, 1, 0]])
    m, cls, post = want["reg_mask"][0], inp["post_classes"][0], inp["post_boxes"][0]
    assert {0, -1, 4} <= set(cls.tolist()) and np.isnan(post).any()
    assert not m[2] and m[1] and m[3] and want["wh"][0, 0, 0] == 4.0 and want["wh"][0, 1, 0] == 4.0     # clipped to 0 and to W - 1
    assert not m[11:15].any() and m[15] and m[16] and 0 < want["wh"][0, 3, 1] <= 1 and want["wh"][0, 16, 1] == 0.75
    assert want["reg"][0, 4].tolist() == [0.0, 0.5] and want["ind"][0, 6] == want["ind"][0, 7] == want["ind"][0, 8]
    for k in KEYS_F32:
        assert not want[k][0, ~m.astype(bool)].any(), k                                   # skipped slots are zero
    for b in want["hm"].reshape(-1, *want["hm"].shape[-2:]):
        assert b.max() in (0.0, 1.0)


KEYS_F32 = ("wh", "reg", "ind")


def test_configs_load_and_build():
    from minddet.models import Config, build_detector

    plain = Config.fromfile(os.path.join(ROOT, "configs", "centernet", "centernet_r18_dcn.py"))
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centernet", "centernet_r18_dcn_train.py"))
    assert cfg.model == plain.model and cfg.test_cfg == plain.test_cfg and plain.train_cfg is None and "neck" not in cfg.model
    assert cfg.model["num_classes"] == 80 and cfg.data["input_hw"] == (512, 512) and cfg.data["down_ratio"] == 4
    tg = det_ops.CenterNetTargets.from_config(cfg)
    assert (tg.num_classes, tg.feature_map_size, tg.max_objs, tg.min_overlap) == (80, (128, 128), 128, 0.7)
    net = build_detector(cfg.model, cfg.train_cfg, cfg.test_cfg)
    assert net.num_classes == 80 and net.n_out == 84
    loss = net.loss_op()
    assert loss is net.loss_op() and isinstance(loss, det_ops.CenterNetLoss)
    at = loss.at
    assert (at.num_classes, at.off_hm, at.off_wh, at.off_reg) == (80, 0, 80, 82)
    assert (at.hm_weight, at.wh_weight, at.off_weight) == (1.0, float(np.float32(0.1)), 1.0)
    assert build_detector(plain.model, plain.train_cfg, plain.test_cfg).loss_op().at.wh_weight == at.wh_weight    # the reference's defaults


def test_radius_is_the_same_under_the_widened_fp32_overlap():
    """the operator widens its fp32 attribute: 0.7f is 0.699999988, not the reference's float64 0.7.  On every integer box size a map up
    to 512 x 512 can give, the truncated radius is the same under both, so the widening cannot change a result there"""
    h, w = np.meshgrid(np.arange(1, 513), np.arange(1, 513), indexing="ij")
    wide = ct.gaussian_radius(h, w, ct.overlap_of(0.7)).astype(np.int64)
    assert np.array_equal(wide, ct.gaussian_radius(h, w, 0.7).astype(np.int64)) and wide.max() > 100
