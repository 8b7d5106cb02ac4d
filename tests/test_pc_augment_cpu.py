"""CPU: the KITTI training augmentation without a GPU -- the ABI of include/minddet_hip_pcaug.h (the functions exported,
the semantic refusals answered before any device call, the ctypes mirrors laid out as the header says), the
contract tests/pcaug_contract.py against the reference's own outputs (tests/golden/pc_augment_vectors.npz, written by
tests/golden/gen_pc_augment.py from noise_per_object, remove_points_in_boxes, the four global steps and
filter_gt_box_outside_range), and det_ops.PointCloudAugment built from both train configs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from minddet_amd import _lib, det_ops
from tests import pcaug_contract as pc
from tests import abi_header as ah
from tests.abi_cases import I, T
from tests.abi_cases_pcaug import CASES, F64, PCBoxes
from tests.abi_derive import both, edited, item, lib_handle, rc, refuse_single_defects, shape
from tests.pcaug_cases import GOLD, NAMES, contract_case, fixture_case, reference_owner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = ah.header("minddet_hip_pcaug.h")
SYMS = ["md_pc_noise_per_object", "md_pc_augment_points", "md_pc_augment_boxes"]
UNDECIDED_CAP = 2e-3      # of the pairs within 1 m of a face (the reference's points_in_rbbox against a float64 judge on 24 boxes x 6 000 points: 2.7e-4)


def test_header_declares_the_symbols_and_the_library_exports_them():
    assert ah.aot_symbols(HDR) == SYMS and '#include "minddet_hip_points.h"' in HDR
    for cite in ("preprocess.py:124-170", ":560-668", ":423-441", ":138-152", "geometry.py:18-55", "box_np_ops.py:390-392"):
        assert cite in HDR, cite
    for quirk in ("(a)", "(b)", "(c)", "(d)", "(e)"):
        assert quirk in HDR
    assert "minddet_hip_pcaug.h" in open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    assert {c.sym for c in CASES} == set(SYMS) and len({c.id for c in CASES}) == len(CASES)
    lib = lib_handle()
    for s in SYMS:
        assert getattr(lib, s)(0, None, None, None, None, None, None) == 1      # wrong parameter count, before anything else
    assert not set(SYMS) & set(_lib.exported_symbols())                          # declared in the new header only


def test_ctypes_mirrors_have_the_headers_layout():
    assert ah.statements("md_pc_boxes_attrs", HDR) == ["float bv_range[4]"]
    for got in (det_ops._PCBoxesAttrs, PCBoxes):
        assert C.sizeof(got) == 16 and got.bv_range.offset == 0 and got.bv_range.size == 16
    for name, macro in (("PCAUG_MAX_BOXES", "MD_PCAUG_MAX_BOXES"), ("PCAUG_MAX_TRIES", "MD_PCAUG_MAX_TRIES")):
        assert getattr(det_ops, name) == ah.defines(HDR)[macro]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_pcaug", case)


def test_semantic_refusals_return_the_documented_codes():
    ARG, SIZE = 2, 4
    noise, noise_null, points, points_ws, boxes = CASES
    for i, e in enumerate([shape(0, (2, 3, 8)), shape(0, (2, 3, 9)), shape(1, (3,), I), shape(2, (2, 4), "uint8"), shape(3, (2, 3, 4, 2), F64),
                           shape(4, (2, 3, 5), F64), shape(5, (2, 3, 5), F64), shape(6, (2, 4), I), shape(7, (2, 3, 3), F64), shape(8, (2, 4, 7)),
                           both(shape(3, (2, 3, 0, 3), F64), shape(4, (2, 3, 0), F64), shape(5, (2, 3, 0), F64))]):     # T < 1
        assert rc(noise, e) == ARG, i
    assert rc(noise_null, shape(0, (2, 3, 8))) == ARG

    def grow_noise(G, Tn, B=2):
        return both(shape(0, (B, G, 7)), shape(1, (B,), I), shape(2, (B, G), "uint8"), shape(3, (B, G, Tn, 3), F64), shape(4, (B, G, Tn), F64),
                     shape(5, (B, G, Tn), F64), shape(6, (B, G), I), shape(7, (B, G, 4), F64), shape(8, (B, G, 7)))

    assert rc(noise, grow_noise(257, 4)) == SIZE and rc(noise, grow_noise(3, 129)) == SIZE and rc(noise, grow_noise(1, 1, 4097)) == SIZE

    for i, e in enumerate([both(shape(0, (300, 5)), shape(10, (300, 5))), shape(0, (300, 3)), shape(1, (4,), I), shape(2, (2, 3, 8)),
                           shape(3, (3,), I), shape(4, (2, 2), "uint8"), shape(5, (2, 3, 3), F64), shape(6, (2, 2, 8)), shape(6, (3, 2, 7)),
                           shape(7, (3,), I), shape(8, (1,), I), shape(9, (2, 5), F64), shape(9, (3, 6), F64), shape(10, (299, 4)),
                           shape(11, (2,), I), shape(12, (301,), I)]):
        assert rc(points, e) == ARG, i

    def part(c):                                          # remove operands given in part
        t = c.operands[7]
        c.operands[7] = T(t.shape, t.dtype, "opt", null=True)
    assert rc(points, part) == ARG
    big = 1 << 30
    call = edited(points, lambda c: None)                             # (the shapes alone say 2^30 points: the host blocks stay small, nothing is touched)
    call.shapes[0], call.shapes[10], call.shapes[12] = [big, 4], [big, 4], [big]
    assert call.run(lib_handle()) == SIZE
    assert rc(points, shape(6, (2, 257, 7))) == SIZE
    assert rc(points_ws, shape(13, (900,), "uint8")) == SIZE                                  # R = 0 here: 908 bytes are used

    nan, inf = float("nan"), float("inf")
    for i, e in enumerate([shape(0, (2, 3, 8)), shape(1, (3,), I), shape(2, (2, 4), "uint8"), shape(3, (2, 4), I), shape(4, (2, 7), F64),
                           shape(5, (2, 4, 7)), shape(6, (3, 3), I), shape(7, (3,), I)]):
        assert rc(boxes, e) == ARG, i
    for k, v in ((0, nan), (1, inf), (2, -inf), (3, nan)):
        assert rc(boxes, item("bv_range", k, v)) == ARG, (k, v)
    grow = both(shape(0, (2, 257, 7)), shape(2, (2, 257), "uint8"), shape(3, (2, 257), I), shape(5, (2, 257, 7)), shape(6, (2, 257), I))
    assert rc(boxes, grow) == SIZE


def test_fixture_carries_what_the_cases_promise():
    z = np.load(GOLD)
    assert sorted(z["cases"]) == sorted(NAMES) and os.path.getsize(GOLD) < 1000 * 1000
    car, nog, ped = (fixture_case(n) for n in NAMES)
    assert car["gt_boxes"].shape == (12, 7) and car["loc"].shape == (12, 100, 3) and car["points"].shape == (3000, 4) and "grot" in car
    assert int((car["valid"] == 0).sum()) == 1 and car["selected"][0] == car["selected"][7] == -1 and not car["loc"][[0, 7]].any()
    assert "grot" not in nog and not bool(nog["enable_grot"])
    assert ped["gt_boxes"].shape == (20, 7) and ped["remove_boxes"].shape == (3, 7) and int(ped["remove_from"]) > 0 and ped["removed"].any()
    assert ped["gt_boxes"][:, 3].min() == np.float32(0.6) and ped["gt_boxes"][:, 4].max() == np.float32(4.6)
    assert {float(f["global"][0]) for f in (car, nog, ped)} == {0.0, 1.0}
    for f in (car, nog, ped):
        assert f["points"].dtype == f["points_translate"].dtype == f["final_boxes"].dtype == np.float32 and f["loc"].dtype == np.float64
        assert (f["selected"] >= 0).sum() >= len(f["selected"]) - 4
    assert sum(int((~f["range_mask"]).sum()) for f in (car, nog, ped)) >= 2
    assert z["collision_a"].shape == (40, 5) and z["collision_a_covers_b"].sum() == 8 and z["collision_b_covers_a"].sum() == 8
    # quirk (a): containment without crossing edges is in the collision case only -- the three scenes were generated with the assertion
    assert (z["collision_a_covers_b"] & ~z["collision_edges"]).any()


@pytest.mark.parametrize("name", NAMES)
def test_contract_decisions_equal_the_reference(name):
    f, c = fixture_case(name), contract_case(name)
    assert np.array_equal(c["selected"], f["selected"])
    p = c["pts"]
    own_ref = reference_owner(f)
    d = p["decided"]
    assert np.array_equal(p["owner"][d], own_ref[d])
    assert p["drop_decided"] and np.array_equal(p["owner"] == -2, own_ref == -2)      # no plant is on a remove box: the kept count is pinned
    near, undecided = int(p["near"].sum()), int((p["margin"] <= pc.MARGIN).sum())
    assert 1 <= undecided <= UNDECIDED_CAP * near, (undecided, near)      # (plants included: every case has one or two, on a face by design)
    b = c["boxes"]
    mask_ref = np.zeros(len(f["valid"]), bool)
    mask_ref[np.flatnonzero(f["valid"])] = f["range_mask"]
    dec = (b["margin"] > pc.MARGIN) & (f["valid"] != 0)
    assert np.array_equal(b["mask"][dec], mask_ref[dec]) and dec.sum() >= f["valid"].sum() - 1


WORST = {}


@pytest.mark.parametrize("name", NAMES)
def test_contract_floats_are_within_the_forward_bound_of_the_reference(name):
    f, c = fixture_case(name), contract_case(name)
    G = len(f["valid"])
    tf_ref = f["obj_transform"]
    e_tf = np.abs(c["tf"] - tf_ref)
    bound_tf = np.zeros((G, 4))
    bound_tf[:, 0] = bound_tf[:, 1] = c["terr"]
    bound_tf[:, 3] = 16 * 2.0 ** -53 * (np.pi + np.abs(tf_ref[:, 3]))
    worst_tf = float((e_tf / np.maximum(bound_tf, 1e-300))[(e_tf > 0)].max()) if (e_tf > 0).any() else 0.0
    assert (e_tf <= bound_tf).all(), worst_tf
    moved_err = np.abs(c["moved"].astype(np.float64) - f["boxes_noise"])
    bound_moved = 2 * pc.U * np.abs(f["boxes_noise"]) + np.stack([c["terr"]] * 7, 1) * (np.arange(7) < 2)
    assert (moved_err <= bound_moved).all()
    p = c["pts"]
    nf, n = int(f["remove_from"]), len(f["points"])
    drop_ref = np.concatenate([np.zeros(nf, bool), f["removed"]]) if len(f["remove_boxes"]) else np.zeros(n, bool)
    keep = p["owner"] != -2
    assert np.array_equal(keep, ~drop_ref)                 # (no point of the fixture is within the margin of a remove box's face)
    masks = f["point_masks"] & (f["valid"] != 0)[None]
    own_ref = np.where(masks.any(1), masks.argmax(1), -1)
    agree = own_ref == p["owner"][keep]                    # an undecided point may have another owner: it is moved differently
    ref = f["points_translate"]
    err = np.abs(p["exact"] - ref[:, :3]).max(1)
    worst_pt = float((err[agree] / p["bound"][agree]).max())
    assert (~agree).sum() <= 8 and (err[agree] <= p["bound"][agree]).all(), worst_pt
    assert np.array_equal(p["points"][:, 3], ref[:, 3])
    b = c["boxes"]
    vi = np.flatnonzero(f["valid"])
    err_b = np.abs(b["all"][vi][:, :6] - f["boxes_translate"][:, :6])
    worst_box = float((err_b / b["bound"][vi][:, :6]).max())
    assert (err_b <= b["bound"][vi][:, :6]).all(), worst_box
    kept = b["keep"][vi]
    if np.array_equal(kept, f["range_mask"]):
        d = np.abs(b["all"][vi][kept][:, 6] - f["final_boxes"][:, 6])
        d = np.minimum(d, np.abs(d - 2 * np.pi))
        assert (d <= b["bound"][vi][kept][:, 6]).all(), float((d / b["bound"][vi][kept][:, 6]).max())
        assert np.array_equal(b["gt_classes"][:b["count"]], f["final_classes"])
        worst_box = max(worst_box, float((d / b["bound"][vi][kept][:, 6]).max()))
    WORST[name] = (worst_tf, worst_pt, worst_box)
    print(f"{name}: worst error / bound: obj_transform {worst_tf:.3f}, points {worst_pt:.3f}, boxes {worst_box:.3f}")
    assert worst_pt > 0 and worst_box > 0


def test_contract_collision_predicate_equals_the_references_parts():
    z = np.load(GOLD)
    A, Bq = z["collision_a"].astype(np.float64), z["collision_b"].astype(np.float64)
    ax, ay = pc.rect(A[:, 2], A[:, 3], A[:, 4])
    bx, by = pc.rect(Bq[:, 2], Bq[:, 3], Bq[:, 4])
    edges, a_b, b_a, hit = pc.collide(ax + A[:, :1], ay + A[:, 1:2], bx + Bq[:, :1], by + Bq[:, 1:2])
    assert np.array_equal(edges, z["collision_edges"]) and np.array_equal(a_b, z["collision_a_covers_b"])
    assert np.array_equal(b_a, z["collision_b_covers_a"])
    assert np.array_equal(hit, z["collision_standup"] & (z["collision_edges"] | z["collision_a_covers_b"] | z["collision_b_covers_a"]))


@pytest.mark.parametrize("name", ("car", "ped_cycle"))
def test_train_configs_build_the_augmentation(name):
    from minddet.models import Config

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", f"pointpillars_{name}_xyres16_train.py"))
    a = cfg.train_cfg["augment"]
    # the values of the reference's car_xyres16.yaml / ped_cycle_xyres16.yaml (:19-23)
    assert list(a["gt_loc_noise_std"]) == [0.25, 0.25, 0.25] and list(a["gt_rotation_noise"]) == [-0.15707963267, 0.15707963267]
    assert list(a["global_rotation_noise"]) == [-0.78539816, 0.78539816] and list(a["global_scaling_noise"]) == [0.95, 1.05]
    assert list(a["global_random_rot_range"]) == [0, 0] and list(a["global_loc_noise_std"]) == [0.2, 0.2, 0.2]
    aug = det_ops.PointCloudAugment.from_config(cfg)
    r = cfg.model["voxel_generator"]["point_cloud_range"]
    assert aug.bv_range == (r[0], r[1], r[3], r[4]) and aug.num_try == 100 and aug.flip_probability == 0.5 and not aug.enable_grot
    assert aug.gt_loc_noise_std == (0.25, 0.25, 0.25)


def test_augment_defaults_and_refused_options():
    aug = det_ops.PointCloudAugment((0, -40, 70, 40))
    assert aug.gt_rotation_noise == (-np.pi / 3, np.pi / 3) and aug.gt_loc_noise_std == (1.0, 1.0, 1.0) and aug.enable_grot
    assert aug.global_random_rot_range == (0.78, 2.35) and aug.global_scaling_noise == (0.95, 1.05) and aug.num_try == 100
    assert det_ops.PointCloudAugment((0, -40, 70, 40), global_random_rot_range=0.25).global_random_rot_range == (-0.25, 0.25)
    assert det_ops.PointCloudAugment((0, -40, 70, 40), shuffle_points=False, group_ids=None).num_try == 100      # named but off: fine
    for k in ("group_ids", "reference_detections", "remove_environment", "remove_outside_points", "without_reflectivity", "bev_only",
              "shuffle_points"):
        with pytest.raises(ValueError):
            det_ops.PointCloudAugment((0, -40, 70, 40), **{k: True})
    with pytest.raises(ValueError):
        det_ops.PointCloudAugment((0, -40, 70, 40), num_try=129)
    with pytest.raises(ValueError):
        det_ops.PointCloudAugment((0, -40, 70, 40), no_such_option=1)
    with pytest.raises(ValueError):                        # boxes wider than 7
        det_ops.pc_noise_per_object(torch.zeros((1, 2, 9)), None, None, None, None)
    assert det_ops.pc_augment_points_workspace_bytes(300, 2, 3, 2) == 1420 <= 1424       # (the library's answer, the header's bound)
