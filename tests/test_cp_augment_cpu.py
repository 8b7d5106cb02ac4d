"""CPU: the CenterPoint training input without a GPU -- the ABI of include/minddet_hip_cpaug.h (the functions exported,
the semantic refusals answered before any device call, the ctypes mirrors laid out as the header says), the
contract tests/cpaug_contract.py against the reference's own outputs (tests/golden/cp_augment_vectors.npz, written by
tests/golden/gen_cp_augment.py from points_count_rbbox, sample_all, the four global steps and filter_gt_box_outside_range),
det_ops.CenterPointAugment built from the train config and its refusals, and the one definition of the collision predicate."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

from minddet_amd import _lib, det_ops
from tests import cpaug_contract as cc
from tests import abi_header as ah
from tests.abi_cases import I, T
from tests.abi_cases_cpaug import CASES, F64, CPBoxes, CPCount
from tests.abi_derive import both, edited, item, lib_handle, rc, refuse_single_defects, shape
from tests.cpaug_cases import GOLD, NAMES, contract_case, fixture_case, has_candidates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = ah.header("minddet_hip_cpaug.h")
SYMS = ["md_cp_aug_count_points", "md_cp_aug_select", "md_cp_aug_points", "md_cp_aug_boxes"]
U8 = "uint8"


def test_header_declares_the_symbols_and_the_library_exports_them():
    assert ah.aot_symbols(HDR) == SYMS and '#include "minddet_hip_points.h"' in HDR
    for cite in ("preprocess.py:46-157, 187-193", "sample_ops.py:127-154, 245-291", "box_np_ops.py:9-14", ":102-116", ":825-827"):
        assert cite in HDR, cite
    assert "minddet_hip_cpaug.h" in open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    assert {c.sym for c in CASES} == set(SYMS) and len({c.id for c in CASES}) == len(CASES)
    lib = lib_handle()
    for s in SYMS:
        assert getattr(lib, s)(0, None, None, None, None, None, None) == 1      # wrong parameter count, before anything else
    assert not set(SYMS) & set(_lib.exported_symbols())                          # declared in the new header only


def test_ctypes_mirrors_and_limits_have_the_headers_layout():
    for name, want in (("md_cp_count_attrs", ["int32_t min_points"]), ("md_cp_boxes_attrs", ["float bv_range[4]"])):
        assert ah.statements(name, HDR) == want
    for got in (det_ops._CPBoxesAttrs, CPBoxes):
        assert C.sizeof(got) == 16 and got.bv_range.offset == 0 and got.bv_range.size == 16
    for got in (det_ops._CPCountAttrs, CPCount):
        assert C.sizeof(got) == 4 and got.min_points.offset == 0
    for name, macro in (("CPAUG_MAX_GT", "MD_CPAUG_MAX_GT"), ("CPAUG_MAX_CAND", "MD_CPAUG_MAX_CAND")):
        assert getattr(det_ops, name) == ah.defines(HDR)[macro]
    assert (det_ops.CPAUG_MAX_GT, det_ops.CPAUG_MAX_CAND) == (512, 256) and "#define MD_CPAUG_MAX_BATCH 4096" in HDR
    assert det_ops.cp_aug_count_points_workspace_bytes(2, 3) == 576 and det_ops.cp_aug_select_workspace_bytes(2, 3, 4) == 64
    assert det_ops.cp_aug_points_workspace_bytes(300, 40, 2) == 480 <= 484              # (the library's answer, the header's bound)


def test_collision_predicate_is_defined_once():
    src = os.path.join(ROOT, "minddet_amd", "csrc")
    defs = {os.path.basename(p): len(re.findall(r"^__device__[^\n;]*\bcollide\(", open(p).read(), flags=re.M))
            for p in glob.glob(os.path.join(src, "*.hip")) + glob.glob(os.path.join(src, "*.h"))}
    assert {k: v for k, v in defs.items() if v} == {"aug_geom.h": 1}
    for name in ("pcaug.hip", "cpaug.hip"):
        text = open(os.path.join(src, name)).read()
        assert '#include "aug_geom.h"' in text and "collide(" in text
        assert text.index("#pragma clang fp contract(off)") < text.index('#include "aug_geom.h"')


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_cpaug", case)


def _null(i):
    def edit(c):
        t = c.operands[i]
        c.operands[i] = T(t.shape, t.dtype, "opt", null=True)
    return edit


def test_semantic_refusals_return_the_documented_codes():
    ARG, SIZE = 2, 4
    count_ws, count, select_ws, select, points_ws, points, boxes, boxes_plain = CASES
    for i, e in enumerate([shape(0, (300, 4)), shape(0, (300, 6)), shape(1, (4,), I), shape(2, (2, 3, 7)), shape(2, (3, 3, 9)), shape(3, (3,), I),
                           shape(4, (2, 4), I), shape(5, (2, 4), U8), shape(5, (3, 3), U8)]):
        assert rc(count, e) == ARG, i
    grow = both(shape(2, (2, 513, 9)), shape(4, (2, 513), I), shape(5, (2, 513), U8))
    assert rc(count, grow) == SIZE
    call = edited(count, lambda c: None)                  # (the shapes alone say 2^30 points: the host blocks stay small, nothing is touched)
    call.shapes[0] = [1 << 30, 5]
    assert call.run(lib_handle()) == SIZE
    assert rc(count_ws, shape(6, (575,), U8)) == SIZE

    for i, e in enumerate([shape(0, (2, 3, 7)), shape(1, (3,), I), shape(2, (2, 4), U8), shape(3, (2, 4, 7)), shape(3, (3, 4, 9)), shape(4, (3,), I),
                           shape(5, (2, 5), I), shape(6, (2, 5), U8)]):
        assert rc(select, e) == ARG, i
    assert rc(select, both(shape(0, (2, 513, 9)), shape(2, (2, 513), U8))) == SIZE
    assert rc(select, both(shape(3, (2, 257, 9)), shape(5, (2, 257), I), shape(6, (2, 257), U8))) == SIZE
    assert rc(select_ws, shape(7, (63,), U8)) == SIZE

    for i, e in enumerate([both(shape(0, (300, 4)), shape(7, (340, 4))), shape(1, (4,), I), shape(2, (40, 4)), shape(3, (8,), I), shape(3, (10,), I),
                           shape(4, (2, 4, 7)), shape(4, (3, 4, 9)), shape(5, (2, 5), U8), shape(6, (2, 6), F64), shape(6, (3, 7), F64),
                           shape(7, (300, 5)), shape(7, (340, 4)), shape(8, (2,), I)]):
        assert rc(points_ws, e) == ARG, i
    for i in (2, 3, 4, 5):                                # candidate operands given in part
        assert rc(points_ws, _null(i)) == ARG, i
    assert rc(points, shape(7, (340, 5))) == ARG        # no candidates: N rows
    call = edited(points, lambda c: None)
    call.shapes[0], call.shapes[7] = [1 << 30, 5], [1 << 30, 5]
    assert call.run(lib_handle()) == SIZE
    assert rc(points_ws, both(shape(3, (2 * 257 + 1,), I), shape(4, (2, 257, 9)), shape(5, (2, 257), U8))) == SIZE
    assert rc(points_ws, shape(9, (479,), U8)) == SIZE                                       # 480 bytes are used

    nan, inf = float("nan"), float("inf")
    for i, e in enumerate([shape(0, (2, 3, 7)), shape(1, (2, 4), I), shape(2, (3,), I), shape(3, (2, 4), U8), shape(4, (2, 4, 7)), shape(5, (2, 5), I),
                           shape(6, (2, 5), U8), shape(7, (2, 6), F64), shape(8, (2, 6, 9)), shape(8, (2, 7, 7)), shape(9, (2, 6), I),
                           shape(10, (3,), I)]):
        assert rc(boxes, e) == ARG, i
    for i in (4, 5, 6):
        assert rc(boxes, _null(i)) == ARG, i
    assert rc(boxes_plain, shape(8, (2, 7, 9))) == ARG
    for k, v in ((0, nan), (1, inf), (2, -inf), (3, nan)):
        assert rc(boxes, item("bv_range", k, v)) == ARG, (k, v)
    grow = both(shape(0, (2, 513, 9)), shape(1, (2, 513), I), shape(3, (2, 513), U8), shape(8, (2, 517, 9)), shape(9, (2, 517), I))
    assert rc(boxes, grow) == SIZE
    grow = both(shape(4, (2, 257, 9)), shape(5, (2, 257), I), shape(6, (2, 257), U8), shape(8, (2, 260, 9)), shape(9, (2, 260), I))
    assert rc(boxes, grow) == SIZE


def test_aliased_outputs_are_refused():
    """an output at the address of an input or of another output: rc 2 before any device call"""
    lib = lib_handle()
    for case, pairs in ((CASES[1], [(4, 3), (5, 4)]), (CASES[3], [(6, 2)]), (CASES[4], [(7, 0), (7, 2), (8, 1)]), (CASES[6], [(8, 0), (9, 1), (10, 2), (10, 9)])):
        for out, other in pairs:
            call = edited(case, lambda c: None)
            n = call.n
            ops = call.case.operands
            bufs = [(C.c_char * 65536)() for _ in range(n)]
            params = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
            params[out] = params[other]
            for i, t in enumerate(ops):
                if t.null:
                    params[i] = None
            ndims = (C.c_int * n)(*[0 if t.null else len(t.shape) for t in ops])
            keep = [(C.c_int64 * max(len(t.shape), 1))(*t.shape) for t in ops]
            shapes = (C.POINTER(C.c_int64) * n)(*[C.cast(k, C.POINTER(C.c_int64)) for k in keep])
            dtypes = (C.c_char_p * n)(*[t.dtype.encode() for t in ops])
            extra = None if case.extra is None else C.byref(case.extra)
            assert getattr(lib, case.sym)(n, params, ndims, shapes, dtypes, None, extra) == 2, (case.id, out, other)


def test_fixture_carries_what_the_cases_promise():
    z = np.load(GOLD)
    assert sorted(z["cases"]) == sorted(NAMES) and os.path.getsize(GOLD) < 1000 * 1000
    n = fixture_case("nusc")
    assert n["gt_boxes"].shape == (14, 9) and int((n["gt_classes"] == 0).sum()) == 3 and n["points"].shape == (3000, 5)
    assert n["cand_boxes"].shape == (12, 9) and sorted(set(n["cand_group"].tolist())) == [0, 1, 2] and int(n["min_points"]) == 5
    assert n["counts"].min() == 0 and n["counts"].max() == 10 and 0 < n["keep"].sum() < 14
    assert n["global"][:2].tolist() == [1.0, 1.0] and np.abs(n["global"][4:]).min() > 0
    flips = {tuple(fixture_case(f"flips{k}")["global"][:2].tolist()) for k in range(3)}
    assert flips == {(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)}
    for k in range(3):
        f = fixture_case(f"flips{k}")
        assert f["gt_boxes"].shape == (6, 9) and f["cand_boxes"].shape == (4, 9) and f["points"].shape == (400, 5)
    o = fixture_case("order")
    assert o["accept"].tolist() == [0, 1, 0, 0, 1, 1, 1, 0, 0, 1, 1] and o["keep"].tolist() == [1, 0] and o["cand_group"].tolist() == [0] * 8 + [1] * 3
    p = fixture_case("plants")
    assert not has_candidates(p) and int(p["face_points"]) == 9 and p["range_rows"].tolist() == [2, 4]
    for name in NAMES:
        f = fixture_case(name)
        assert f["points"].dtype == f["points_translate"].dtype == f["final_boxes"].dtype == np.float32 and f["global"].dtype == np.float64
        assert f["global"].shape == (7,) and ((~f["range_mask"]).any() or name == "order")      # (order: every row stays in range)
        if has_candidates(f):
            assert 0 < f["accept"].sum() < len(f["accept"]) and f["cand_offsets"][-1] == len(f["cand_points"])


@pytest.mark.parametrize("name", NAMES)
def test_contract_decisions_equal_the_reference(name):
    f, c = fixture_case(name), contract_case(name)
    cnt = c["count"]
    if name == "plants":
        und = {(int(i), int(g)) for i, g in zip(*np.nonzero(cnt["margin"] <= cc.MARGIN))}
        assert und == {(i, 0) for i in range(9)} and not cnt["decided"]
        assert set(np.flatnonzero(c["boxes"]["margin"] <= cc.MARGIN).tolist()) == {2, 4}
    else:
        assert cnt["decided"] and np.array_equal(cnt["counts"], f["counts"]) and (c["boxes"]["margin"] > cc.MARGIN).all()
    assert ((f["counts"] >= cnt["lo"]) & (f["counts"] <= cnt["hi"])).all()
    kd = cnt["keep_decided"]
    assert kd.all() and np.array_equal(cnt["keep"], f["keep"])
    if has_candidates(f):
        assert np.array_equal(c["accept"], f["accept"])
    b = c["boxes"]
    dec = b["margin"] > cc.MARGIN
    assert len(b["mask"]) == len(f["range_mask"]) and np.array_equal(b["mask"][dec], f["range_mask"][dec])
    assert np.array_equal(b["gt_classes"][:b["count"]][dec[b["mask"]]], f["classes_merged"][b["mask"]][dec[b["mask"]]])
    if dec.all():
        assert b["count"] == len(f["final_boxes"]) and np.array_equal(b["gt_classes"][:b["count"]], f["final_classes"])
        assert not b["gt_boxes"][b["count"]:].any() and not b["gt_classes"][b["count"]:].any()


@pytest.mark.parametrize("name", NAMES)
def test_contract_floats_are_within_the_forward_bound_of_the_reference(name):
    f, c = fixture_case(name), contract_case(name)
    p, b = c["pts"], c["boxes"]
    ref = f["points_translate"]
    assert ref.shape == p["points"].shape and np.array_equal(p["points"][:, 3:], ref[:, 3:])      # columns 3 and up: bit for bit
    if has_candidates(f):
        assert p["n_cand"] == int(sum(np.diff(f["cand_offsets"])[f["accept"] != 0])) > 0
    err = np.abs(p["exact"] - ref[:, :3]).max(1)
    worst_pt = float((err / p["bound"]).max())
    assert (err <= p["bound"]).all(), worst_pt
    err_b = np.abs(b["all"] - f["boxes_translate"])
    err_b[:, 8] = np.minimum(err_b[:, 8], np.abs(err_b[:, 8] - 2 * np.pi))
    worst_box = float((err_b / np.maximum(b["bound"], 1e-300)).max())
    assert (err_b <= b["bound"]).all(), worst_box
    print(f"{name}: worst error / bound: points {worst_pt:.3f}, boxes {worst_box:.3f}")
    assert (worst_pt > 0 and worst_box > 0) or name == "plants"      # (plants: the identity transform, nothing is rounded)
    # every stage the reference stored is the float64 stage rounded, within the final bound (the stages' own bounds are smaller)
    assert np.array_equal(f["points_merged"][p["n_cand"]:], f["points"])


def test_train_config_builds_the_augmentation():
    from minddet.models import Config

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc_train.py"))
    a = cfg.train_cfg["augment"]
    assert list(a["global_rot_noise"]) == [-0.3925, 0.3925] and list(a["global_scale_noise"]) == [0.95, 1.05]
    assert a["global_translate_std"] == 0 and a["min_points_in_gt"] == -1 and cfg.train_cfg["max_voxel_num"] == 30000
    aug = det_ops.CenterPointAugment.from_config(cfg)
    r = cfg.model["voxel_generator"]["range"]
    assert aug.bv_range == (r[0], r[1], r[3], r[4]) and aug.global_rot_noise == (-0.3925, 0.3925) and aug.global_scale_noise == (0.95, 1.05)
    assert aug.global_translate_std == (0.0, 0.0, 0.0) and aug.min_points_in_gt == -1
    tiny = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_tiny_points_train.py"))
    assert tiny.model["type"] == "PillarDetector" and len(tiny.train_cfg["assigner"]["target_assigner"]["tasks"]) == 2
    assert tiny.train_cfg["assigner"]["max_objs"] == 32 and det_ops.voxel_grid(tiny.model["voxel_generator"]["voxel_size"],
                                                                               tiny.model["voxel_generator"]["range"])[:2] == (64, 64)
    assert det_ops.CenterPointAugment.from_config(tiny).min_points_in_gt == 2


def test_augment_refused_options():
    bv, ok = (-51.2, -51.2, 51.2, 51.2), dict(global_rot_noise=[-0.3925, 0.3925], global_scale_noise=[0.95, 1.05])
    aug = det_ops.CenterPointAugment(bv, **ok)
    assert aug.global_translate_std == (0.0, 0.0, 0.0) and aug.min_points_in_gt == -1
    assert det_ops.CenterPointAugment(bv, 0.3, [0.9, 1.1]).global_rot_noise == (-0.3, 0.3)
    # named but off: fine
    assert det_ops.CenterPointAugment(bv, shuffle_points=False, flip_coor=None, global_random_rotation_range_per_object=[0, 0], **ok).bv_range == bv
    for k, v in (("shuffle_points", True), ("flip_coor", 0.5), ("use_group_sampling", True), ("group_ids", [1]), ("random_crop", True),
                 ("global_random_rotation_range_per_object", [-0.1, 0.1]), ("no_such_option", 1)):
        with pytest.raises(ValueError):
            det_ops.CenterPointAugment(bv, **{k: v}, **ok)
    assert "order-dependent" in det_ops.CenterPointAugment.__doc__ and "keyed sort" in det_ops.CenterPointAugment.__doc__
    with pytest.raises(ValueError):                        # boxes that are not 9 wide
        det_ops.cp_aug_select(torch.zeros((1, 2, 7)), None, None, torch.zeros((1, 2, 9)), None, None)
    with pytest.raises(ValueError):                        # points that are not 5 wide
        det_ops.cp_aug_count_points(torch.zeros((4, 4)), None, torch.zeros((1, 2, 9)), None)
    with pytest.raises(ValueError):                        # candidate operands given in part
        det_ops.cp_aug_points(torch.zeros((4, 5)), torch.zeros(2, dtype=torch.int32), torch.zeros((1, 7)), cand_points=torch.zeros((3, 5)))
