"""CPU: the CenterPoint training targets without a GPU -- the ABI of include/minddet_hip_cptargets.h (the function exported,
the semantic refusals answered before any device call, the ctypes mirrors laid out as the header says), the
contract tests/cp_targets_contract.py against the reference's own outputs (tests/golden/cp_target_vectors.npz, written by
tests/golden/gen_cp_targets.py from AssignLabel), the accuracy condition of the GPU test met by the reference itself, and the config."""
import ctypes as C
import os

import numpy as np
import pytest

from minddet_amd import det_ops
from tests import cp_targets_contract as ct
from tests import abi_header as ah
from tests.abi_cases import I
from tests.abi_cases_cptargets import CASES, CPTargets
from tests.abi_derive import attr, both, item, lib_handle, rc, refuse_single_defects, shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = ah.header("minddet_hip_cptargets.h")
GOLD = os.path.join(ROOT, "tests", "golden", "cp_target_vectors.npz")
NAMES = ("small", "tiles", "plants")


def fixture_case(name):
    """-> (gt_boxes, gt_classes, keyword arguments of the contract / of det_ops.cp_assign_targets minus `tasks`, the reference's outputs)"""
    z = np.load(GOLD)
    kw = dict(voxel_size=tuple(float(v) for v in z["voxel_size"]), pc_range=tuple(float(v) for v in z[name + "_pc_range"]),
              out_size_factor=int(z["out_size_factor"]), gaussian_overlap=float(z["gaussian_overlap"]), min_radius=int(z["min_radius"]),
              max_objs=int(z[name + "_max_objs"]), feature_map_size=tuple(int(v) for v in z[name + "_feature_map_size"]))
    want = {k: z[name + "_" + k] for k in ct.KEYS}
    return z[name + "_gt_boxes"], z[name + "_gt_classes"], [int(v) for v in z[name + "_num_classes"]], kw, want


def test_header_declares_the_symbol_and_the_library_exports_it():
    assert ah.aot_symbols(HDR) == ["md_cp_assign_targets"] and '#include "minddet_hip.h"' in HDR
    assert "preprocess.py:285-521" in HDR and "center_utils.py:16-" in HDR
    assert "minddet_hip_cptargets.h" in open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    assert {c.sym for c in CASES} == {"md_cp_assign_targets"} and len({c.id for c in CASES}) == len(CASES)
    lib = lib_handle()
    assert lib.md_cp_assign_targets(0, None, None, None, None, None, None) == 1      # wrong parameter count, before anything else


def test_ctypes_mirrors_have_the_headers_layout():
    want = ah.struct_of("md_cp_targets_attrs", HDR)
    assert C.sizeof(want) == 16 * 4
    for got in (det_ops._CPTargetsAttrs, CPTargets):
        assert ah.same_layout(got, want), got


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_cptargets", case)


def test_semantic_refusals_return_the_documented_codes():
    ARG, SIZE = 2, 4
    case = CASES[0]

    nan, inf = float("nan"), float("inf")
    edits = [
        both(shape(0, (1, 5, 9)), shape(1, (1, 5), I)),                                   # G > M: the reference's assertion
        item("num_classes", 1, 3), item("num_classes", 1, 1), item("num_classes", 0, 0),  # C != max(num_classes), a task without classes
        attr("num_tasks", 0), attr("num_tasks", 9), attr("num_tasks", 1), attr("num_tasks", 3),
        item("voxel_size", 0, nan), item("voxel_size", 1, 0.0), item("voxel_size", 0, -0.2), item("voxel_size", 1, inf),
        item("pc_range", 0, nan), item("pc_range", 1, inf), attr("out_size_factor", 0), attr("out_size_factor", -4),
        attr("gaussian_overlap", nan), attr("gaussian_overlap", 0.0), attr("gaussian_overlap", 1.0), attr("gaussian_overlap", -0.1),
        attr("min_radius", -1),
        shape(0, (1, 3, 8)), shape(0, (2, 3, 9)), shape(1, (1, 4), I), shape(2, (1, 3, 2, 8, 12)), shape(2, (1, 2, 1, 8, 12)),
        shape(2, (2, 2, 2, 8, 12)), shape(3, (1, 2, 4, 9)), shape(3, (1, 2, 5, 10)), shape(4, (1, 2, 5), I), shape(5, (1, 3, 4), "uint8"),
        shape(6, (2, 2, 4), I), shape(7, (1, 5, 10)), shape(7, (1, 4, 9)),
    ]
    for i, e in enumerate(edits):
        assert rc(case, e) == ARG, i
    big = 1100                                                                            # G above the LDS bound (M as large: not rc 2)
    grow = both(shape(0, (1, big, 9)), shape(1, (1, big), I), shape(3, (1, 2, big, 10)), shape(4, (1, 2, big), I), shape(5, (1, 2, big), "uint8"),
                shape(6, (1, 2, big), I), shape(7, (1, big, 10)))
    assert rc(case, grow) == SIZE


@pytest.mark.parametrize("name", NAMES)
def test_contract_equals_the_reference(name):
    boxes, classes, ncs, kw, want = fixture_case(name)
    got = ct.assign(boxes, classes, num_classes=ncs, **kw)
    for k in ("ind", "mask", "cat"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    for k in ("hm", "anno_box", "gt_boxes_and_cls"):                                      # bit for bit
        assert got[k].shape == want[k].shape and np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), k


def test_fixture_carries_what_the_cases_promise():
    z = np.load(GOLD)
    assert sorted(z["cases"]) == sorted(NAMES) and int(str(z["numpy_version"]).split(".")[0]) >= 2
    assert os.path.getsize(GOLD) < 200 * 1024
    boxes, classes, ncs, kw, want = fixture_case("small")
    assert boxes.shape == (2, 24, 9) and kw["feature_map_size"] == (24, 20) and ncs == [1, 2, 2] and kw["max_objs"] == 32
    assert want["hm"].shape == (2, 3, 2, 20, 24) and int((classes[1] > 0).sum()) == 9
    shared = 0
    for i, m in zip(want["ind"].reshape(-1, 32), want["mask"].reshape(-1, 32)):
        _, n = np.unique(i[m > 0], return_counts=True)
        shared += int(n[n > 1].sum())
    assert 4 * shared <= int(want["mask"].sum())                                          # what the GPU round trip may leave out
    boxes, classes, ncs, kw, want = fixture_case("tiles")
    assert kw["feature_map_size"] == (72, 40) and want["hm"].shape == (1, 2, 2, 40, 72)
    corners = want["hm"][0, 0, 0][[0, 0, -1, -1], [0, -1, 0, -1]]
    assert (corners > 0).all() and (want["hm"][0, :, :, :, 63:65] > 0).any() and (want["hm"][0, :, :, 15:17] > 0).any()
    boxes, classes, ncs, kw, want = fixture_case("plants")
    m = want["mask"][0]
    assert 0 < m.sum() < (want["gt_boxes_and_cls"][0, :, 9] > 0).sum()                    # skipped members are listed, not drawn
    assert (want["anno_box"][0][m > 0][:, :2] < 0).any()                                  # the centre just below the range is drawn
    assert {0, 4, -1} <= set(classes[0].tolist()) and (boxes[0, :, 3] == 0).any() and (boxes[0, :, 4] < 0).any()
    assert np.abs(want["gt_boxes_and_cls"][0, :, 6]).max() <= np.float32(np.pi) + 1e-6    # headings wrapped
    for b in want["hm"].reshape(-1, *want["hm"].shape[-2:]):
        assert b.max() in (0.0, 1.0)


@pytest.mark.parametrize("name", NAMES)
def test_reference_meets_the_accuracy_condition_of_the_gpu_test(name):
    """the logs within 4 fp32 ulp, sin / cos within max(4 ulp, 2^-24) of the float64 value of the fp32 input: the reference's own
    anno_box passes the condition the device result is held to"""
    boxes, classes, ncs, kw, want = fixture_case(name)
    rows = ct.slot_rows(want["mask"].shape, classes, ncs)
    worst_log, worst_ratio, _ = ct.transcendental_errors(want["anno_box"], want["mask"], want["gt_boxes_and_cls"], rows)
    assert worst_log <= 4.0 and worst_ratio <= 1.0, (worst_log, worst_ratio)


def test_train_config_builds_the_assigner():
    from minddet.models import Config

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc_train.py"))
    pts = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc_points.py"))
    assert cfg.model == pts.model and cfg.test_cfg == pts.test_cfg and pts.train_cfg is None
    a = cfg.train_cfg["assigner"]
    assert (a["gaussian_overlap"], a["max_objs"], a["min_radius"], a["out_size_factor"]) == (0.1, 500, 2, 4)
    assert a["target_assigner"]["tasks"] == cfg.model["bbox_head"]["tasks"]
    tg = det_ops.CenterPointTargets.from_config(cfg)
    assert tg.feature_map_size == (128, 128) and tg.max_objs == 500 and tg.min_radius == 2 and tg.out_size_factor == 4
    assert tg.gaussian_overlap == 0.1 and tg.pc_range == (-51.2, -51.2) and tg.voxel_size == (0.2, 0.2)
    assert det_ops._task_num_classes(tg.tasks) == [1, 2, 2, 1, 2, 2]
    with pytest.raises(ValueError):
        det_ops.cp_assign_targets(None, None, tasks=[1] * 9, voxel_size=(0.2, 0.2), pc_range=(0, 0), out_size_factor=4, gaussian_overlap=0.1,
                                  min_radius=2, max_objs=4, feature_map_size=(4, 4))
