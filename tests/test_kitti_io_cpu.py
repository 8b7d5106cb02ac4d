"""CPU: the KITTI camera-frame ends without a GPU -- the ABI of include/minddet_hip_kitti.h (the three functions exported, header and
Makefile wired, every documented rc 2 / rc 4 answered before any device call, the ctypes mirror laid out
as the header says), det_ops.KittiCalibration's frustums and the contract tests/kitti_io_contract.py against the reference's own
outputs (tests/golden/kitti_io_vectors.npz, written by tests/golden/gen_kitti_io.py), the contract's rows against
minddet_amd/kitti_eval.py's host path within the derived bound, rows_to_annos, the two configs and the refused options."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from minddet_amd import _lib, det_ops, kitti_eval
from tests import kitti_io_contract as kc
from tests import abi_header as ah
from tests.abi_cases import I
from tests.abi_cases_kitti import CASES, F64, KittiRows   # noqa: F401
from tests.abi_derive import attr, both, edited, item, lib_handle, rc, refuse_single_defects, shape
from tests.kitti_io_cases import CAR_RANGE, GOLD, boxes_as_hulls, calibration, detections, fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["md_pc_crop_hulls", "md_kitti_boxes_to_lidar", "md_kitti_rows"]
U8 = "uint8"
ARG, SIZE = 2, 4


def _hdr():
    return ah.header("minddet_hip_kitti.h")


def test_header_declares_the_symbols_and_the_library_exports_them():
    hdr = _hdr()
    assert ah.aot_symbols(hdr) == SYMS and '#include "minddet_hip_points.h"' in hdr
    for cite in ("box_np_ops.py:625-636", "preprocess.py:59-67", "box_np_ops.py:599-613", "predict.py:204-262, 331-396", "geometry.py:46-54",
                 "remove_environment", "random_crop", "generate_single_sample_dict", "fp32-calibration"):
        assert cite in hdr, cite
    mk = open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    assert "minddet_hip_kitti.h" in mk and os.path.exists(os.path.join(ROOT, "minddet_amd", "csrc", "kitti.hip"))
    assert {c.sym for c in CASES} == set(SYMS) and len({c.id for c in CASES}) == len(CASES)
    lib = lib_handle()
    for sym in SYMS:
        assert getattr(lib, sym)(0, None, None, None, None, None, None) == 1      # wrong parameter count, before anything else
        assert sym not in _lib.exported_symbols()                                  # declared in the new header only
    old = ah.header("minddet_hip_pcaug.h")       # its note stays true of those ops
    assert "reference_detections, remove_environment, remove_outside_points" in old


def test_ctypes_mirror_limits_and_workspace_have_the_headers_layout():
    hdr = _hdr()
    assert ah.statements("md_kitti_rows_attrs", hdr) == ["float limit_range[6]", "int32_t use_limit", "int32_t lidar_input"]
    for got in (det_ops._KittiRowsAttrs, KittiRows):
        assert C.sizeof(got) == 32 and got.limit_range.offset == 0 and got.limit_range.size == 24
        assert got.use_limit.offset == 24 and got.lidar_input.offset == 28 and got.lidar_input.size == 4
    for name, macro in (("CROP_MAX_HULLS", "MD_CROP_MAX_HULLS"), ("CROP_MAX_BATCH", "MD_CROP_MAX_BATCH"), ("KITTI_MAX_DETS", "MD_KITTI_MAX_DETS"),
                        ("KITTI_MAX_LABELS", "MD_KITTI_MAX_LABELS"), ("KITTI_MAX_BATCH", "MD_KITTI_MAX_BATCH")):
        assert getattr(det_ops, name) == ah.defines(hdr)[macro]
    assert det_ops.CROP_MAX_HULLS == kc.MAX_HULLS == 64 and det_ops.KITTI_MAX_DETS == kc.MAX_DETS == 512
    assert "192 B K + 4 (N / 256 + 3) bytes" in hdr
    assert det_ops.crop_hulls_workspace_bytes(300, 2, 3) == 1164 <= 1168 and det_ops.crop_hulls_workspace_bytes(480000, 4, 1) == 8272 <= 768 + 4 * 1878


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_kitti", case)


def test_semantic_refusals_return_the_documented_codes():
    ws, pool, lidar, rows, _ = CASES
    # md_pc_crop_hulls: F != 4, every extent that disagrees
    for i, e in enumerate([shape(0, (300, 3)), shape(0, (300, 5)), shape(1, (2,), I), shape(1, (4,), I), shape(2, (3, 3, 8, 3), F64),
                           shape(2, (2, 3, 7, 3), F64), shape(2, (2, 3, 8, 4), F64), shape(3, (3,), I), shape(4, (299, 4)), shape(4, (300, 3)),
                           shape(5, (2,), I), shape(6, (299,), U8), shape(6, (301,), U8)]):
        assert rc(ws, e) == ARG, i
    K1, B1 = det_ops.CROP_MAX_HULLS + 1, det_ops.CROP_MAX_BATCH + 1
    assert rc(pool, shape(2, (2, K1, 8, 3), F64)) == SIZE
    assert rc(pool, both(shape(1, (B1 + 1,), I), shape(2, (B1, 1, 8, 3), F64), shape(3, (B1,), I), shape(5, (B1 + 1,), I))) == SIZE
    call = edited(pool, lambda c: None)                       # (the shapes alone say 2^30 points: the host blocks stay small, nothing is touched)
    call.shapes[0], call.shapes[4], call.shapes[6] = [1 << 30, 4], [1 << 30, 4], [1 << 30]
    assert call.run(lib_handle()) == SIZE
    assert rc(ws, shape(7, (1159,), U8)) == SIZE            # 1160 bytes are used
    # md_kitti_boxes_to_lidar
    for i, e in enumerate([shape(0, (2, 5, 6)), shape(0, (2, 5, 8)), shape(1, (3,), I), shape(2, (2, 3, 4), F64), shape(2, (2, 4, 3), F64),
                           shape(2, (3, 4, 4), F64), shape(3, (2, 4, 7)), shape(3, (2, 5, 6))]):
        assert rc(lidar, e) == ARG, i
    G1, B2 = det_ops.KITTI_MAX_LABELS + 1, det_ops.KITTI_MAX_BATCH + 1
    assert rc(lidar, both(shape(0, (2, G1, 7)), shape(3, (2, G1, 7)))) == SIZE
    assert rc(lidar, both(shape(0, (B2, 1, 7)), shape(1, (B2,), I), shape(2, (B2, 4, 4), F64), shape(3, (B2, 1, 7)))) == SIZE
    # md_kitti_rows
    for i, e in enumerate([shape(0, (2, 5, 8)), shape(0, (2, 5, 10)), shape(1, (3,), I), shape(2, (2, 3, 4), F64), shape(3, (2, 4, 3), F64),
                           shape(3, (3, 4, 4), F64), shape(4, (2, 3), I), shape(4, (3, 2), I), shape(5, (2, 5, 13)), shape(5, (2, 4, 14)),
                           shape(6, (2, 4), I), shape(6, (3, 5), I), shape(7, (3,), I)]):
        assert rc(rows, e) == ARG, i
    for field, v in (("use_limit", 2), ("use_limit", -1), ("lidar_input", 2), ("lidar_input", -1)):
        assert rc(rows, attr(field, v)) == ARG, (field, v)
    assert rc(rows, item("limit_range", 4, float("nan"))) == ARG
    M1 = det_ops.KITTI_MAX_DETS + 1
    assert rc(rows, both(shape(0, (2, M1, 9)), shape(5, (2, M1, 14)), shape(6, (2, M1), I))) == SIZE
    assert rc(rows, both(shape(0, (B2, 1, 9)), shape(1, (B2,), I), shape(2, (B2, 4, 4), F64), shape(3, (B2, 4, 4), F64), shape(4, (B2, 2), I),
                           shape(5, (B2, 1, 14)), shape(6, (B2, 1), I), shape(7, (B2,), I))) == SIZE


def test_aliased_outputs_are_refused():
    """an output at the address of an input or of another output: rc 2 before any device call"""
    lib = lib_handle()
    for case, pairs in ((CASES[0], ((4, 0), (5, 1), (6, 5), (5, 3), (6, 4))), (CASES[2], ((3, 0),)), (CASES[3], ((5, 0), (6, 4), (7, 1), (7, 6), (6, 5)))):
        for out, other in pairs:
            call = edited(case, lambda c: None)
            n, ops = call.n, call.case.operands
            bufs = [(C.c_char * 65536)() for _ in range(n)]
            params = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
            params[out] = params[other]
            ndims = (C.c_int * n)(*[len(t.shape) for t in ops])
            keep = [(C.c_int64 * max(len(t.shape), 1))(*t.shape) for t in ops]
            shapes = (C.POINTER(C.c_int64) * n)(*[C.cast(k, C.POINTER(C.c_int64)) for k in keep])
            dtypes = (C.c_char_p * n)(*[t.dtype.encode() for t in ops])
            extra = None if case.extra is None else C.byref(case.extra)
            assert getattr(lib, case.sym)(n, params, ndims, shapes, dtypes, None, extra) == 2, (case.sym, out, other)


def test_fixture_carries_what_the_cases_promise():
    z = fixture()
    assert os.path.getsize(GOLD) < 400 * 1000
    for c in (0, 1):
        assert z[f"cal{c}_rect"].dtype == z[f"cal{c}_trv2c"].dtype == z[f"cal{c}_p2"].dtype == np.float64
        assert z[f"cloud{c}"].dtype == np.float32 and z[f"cloud{c}"].shape[1] == 4 and len(z[f"cloud{c}"]) <= 20000
        r = z[f"cal{c}_trv2c"][:3, :3]
        assert np.abs(r @ r.T - np.eye(3)).max() < 1e-12 and np.abs(r).max() < 0.99999 and (z[f"cal{c}_p2"][:3, 3] != 0).all()      # a real rotation; P2's translation
        m = z[f"rop{c}_mask"]
        assert 0.1 * len(m) < m.sum() < 0.4 * len(m) and z[f"rop{c}_surfaces"].shape == (1, 6, 4, 3)
        assert (z[f"cloud{c}"][:, 0] < 0).sum() > 0.3 * len(m)                                                                   # points behind the camera
    assert z["cal0_image_shape"].tolist() != z["cal1_image_shape"].tolist()
    assert z["det_masks"].shape == (len(z["cloud0"]), 3) and z["det_frustums"].shape == (3, 8, 3)
    names = z["plant_names"].tolist()
    assert names == ["on a side face", "on an edge", "at the near face", "just inside far_clip", "beyond far_clip", "behind the camera"]
    assert z["plant_mask"].tolist() == [True, False, True, True, False, False] and not z["plant_open"].any()


@pytest.mark.parametrize("c", (0, 1))
def test_calibration_frustums_equal_the_references(c):
    z = fixture()
    cal = calibration((c,))
    got = cal.image_frustum_host()
    want = z[f"rop{c}_frustum"]
    assert got.shape == (1, 1, 8, 3) and np.abs(got[0, 0] - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(cal.lidar2cam[0] - z[f"cal{c}_rect"] @ z[f"cal{c}_trv2c"]).max() == 0
    assert np.abs(cal.cam2lidar[0] @ cal.lidar2cam[0] - np.eye(4)).max() < 1e-12
    assert np.array_equal(want[kc.SURFACES], z[f"rop{c}_surfaces"][0])                                                       # the contract's table is the reference's
    if c == 0:
        hulls, count = cal.detection_frustums_host(z["det_bboxes"][None])
        assert count.tolist() == [3] and np.abs(hulls[0] - z["det_frustums"]).max() <= 1e-12 * np.abs(z["det_frustums"]).max()
        hulls, count = cal.detection_frustums_host(z["det_bboxes"][None], [2])
        assert count.tolist() == [2] and hulls.shape == (1, 3, 8, 3)
    both = calibration((0, 1))
    assert both.image_frustum().shape == (2, 1, 8, 3) and both.image_frustum().dtype == torch.float64 and both.image_frustum() is both.image_frustum()
    assert np.array_equal(both.image_frustum_host()[c], got[0])
    assert both.tensor("image_shape").dtype == torch.int32 and both.tensor("cam2lidar").shape == (2, 4, 4)


@pytest.mark.parametrize("c", (0, 1))
def test_contract_crop_equals_the_reference(c):
    """the masks exactly, on every row, the planted ones by name; no seeded row is open"""
    z = fixture()
    pts, mask = z[f"cloud{c}"], z[f"rop{c}_mask"]
    out = kc.crop_hulls(pts, [0, len(pts)], z[f"rop{c}_frustum"][None, None], [1])
    assert not out["open"].any() and np.array_equal(out["keep"].astype(bool), mask)
    assert out["offsets"].tolist() == [0, int(mask.sum())] and kc.same_bits(out["points"][:mask.sum()], pts[mask]) and not out["points"][mask.sum():].any()
    if c == 0:
        for row, name, want in zip(z["plant_rows"], z["plant_names"], z["plant_mask"]):
            assert bool(out["keep"][row]) == bool(want), name
        m, op = kc.inside(pts, z["det_frustums"])
        assert np.array_equal(m, z["det_masks"]) and not op.any()
        det = kc.crop_hulls(pts, [0, len(pts)], z["det_frustums"][None], [3])
        assert np.array_equal(det["keep"].astype(bool), z["det_masks"].any(-1))
        two = kc.crop_hulls(pts, [0, len(pts)], z["det_frustums"][None], [2])
        assert np.array_equal(two["keep"].astype(bool), z["det_masks"][:, :2].any(-1))
        none = kc.crop_hulls(pts, [0, len(pts)], z["det_frustums"][None], [0])
        assert not none["keep"].any() and none["offsets"].tolist() == [0, 0]                      # masks.any(-1) over zero columns


def test_contract_margins_and_decisions_on_hand_made_hulls():
    rng = np.random.default_rng(3)
    hulls = boxes_as_hulls(rng, 1, 4)
    centres = hulls[0].mean(1)
    m, op = kc.inside(centres.astype(np.float32), hulls[0])
    assert m.diagonal().all() and not op.diagonal().any()                                         # the corner order gives inward normals
    unit = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1], [1, 1, 0]], np.float64)      # the unit cube in that order
    pts = np.array([[0.5, 0.5, 0.5], [0.0, 0.5, 0.5], [1.0, 0.5, 0.5], [0.5, 0.5, 1.0], [np.nan, 0.5, 0.5], [0.5, 0.5, np.nextafter(np.float32(1), np.float32(0))],
                    [2.0, 0.0, 0.5]], np.float32)
    m, op = kc.inside(pts, unit[None])
    assert m[:, 0].tolist() == [True, False, False, False, True, True, False]                     # on a face is outside (strict); a NaN is outside of nothing
    assert op[:, 0].tolist() == [False, True, True, True, False, False, False]                    # exactly on a face: open; beside a face by one fp32 step: not
    far = kc.crop_hulls(pts, [1, 6], np.stack([unit, unit + 5])[None], [9])                       # a count above K is clamped; rows outside the offsets belong to no sample
    assert far["keep"].tolist() == [0, 0, 0, 0, 1, 1, 0] and far["offsets"].tolist() == [0, 2]


@pytest.mark.parametrize("c", (0, 1))
def test_contract_lidar_boxes_equal_the_reference(c):
    z = fixture()
    cal = calibration((c,))
    lab, ref = z[f"lab{c}_cam"], z[f"lab{c}_lidar"]
    got, xyz = kc.boxes_to_lidar(lab[None], [len(lab)], cal.cam2lidar)
    assert np.abs(xyz[0] - ref[:, :3]).max() <= 64 * kc.U * np.abs(ref[:, :3]).max()              # the float64 values: the sum's order only
    assert kc.same_bits(got[0, :, 3:], ref[:, 3:].astype(np.float32))                             # w, l, h, r: the input bits, reordered
    steps = kc.ulp_steps(got[0], ref.astype(np.float32))
    # measured when the fixture was written: 0 of 168 values differ from the reference's own fp32 result; the cap is one ulp
    assert steps.max() <= 1 and (steps == 1).sum() == 0
    short, _ = kc.boxes_to_lidar(lab[None], [5], cal.cam2lidar)
    assert kc.same_bits(short[0, :5], got[0, :5]) and not short[0, 5:].any()


def _host_annos(dets, count, cal, limit, lidar_input, names):
    preds = []
    for b in range(len(dets)):
        d = dets[b, :min(max(int(count[b]), 0), dets.shape[1])]
        preds.append(kitti_eval.lidar_boxes_to_prediction(d[:, :7], d[:, 8], d[:, 7], cal.rect[b], cal.trv2c[b], cal.p2[b], 100 + b))
    return kitti_eval.predictions_to_kitti_annos(preds, cal.image_shape, names, limit, lidar_input)


def compare_annos(got, want, bounds, what=""):
    """annotation dicts of rows_to_annos against the host path's, per sample within (bbox_bound [n,4], loc_bound [n,3]) of the kept rows"""
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g["name"].tolist() == w["name"].tolist(), (what, b)
        assert set(g) == set(w) and g["image_idx"].tolist() == w["image_idx"].tolist()
        n = len(g["name"])
        if n == 0:
            continue
        bb, lb = bounds[b]
        f32 = lambda v: kc.U32 * np.abs(v)                    # the row is stored as fp32
        assert (np.abs(g["bbox"] - w["bbox"]) <= bb + f32(w["bbox"])).all(), (what, b, np.abs(g["bbox"] - w["bbox"]).max())
        assert (np.abs(g["location"] - w["location"]) <= lb + f32(w["location"])).all(), (what, b)
        assert (np.abs(g["alpha"] - w["alpha"]) <= 8 * kc.U * 8 + f32(w["alpha"])).all(), (what, b)
        for k in ("dimensions", "rotation_y", "score", "truncated", "occluded"):
            assert np.array_equal(np.asarray(g[k], np.float64), np.asarray(w[k], np.float64)), (what, b, k)


def host_bounds(dets, c, cal):
    out = []
    for b in range(len(dets)):
        kept = c["src"][b, :c["count"][b]]
        bb, lb = kc.host_path_bound(dets[b, kept], cal.lidar2cam[b], cal.p2[b])
        out.append((bb, lb))
    return out


@pytest.mark.parametrize("limit,lidar_input", [(CAR_RANGE, False), (None, False), (CAR_RANGE, True)])
def test_contract_rows_agree_with_the_host_path_within_the_derived_bound(limit, lidar_input):
    cal = calibration((0, 1))
    dets = detections(5, 2, 40, cal)
    dets[0, 3, 0], dets[0, 4, :2], dets[1, 5, :3] = 75.0, (60.0, -41.0), (40.0, 2.0, 6.0)      # outside the centre range in x, y, z; inside the image
    dets[0, 6, :2] = (10.0, 30.0)                                           # far to the left of the image
    dets[1, 7, :2] = (12.0, -40.5)                                          # to the right of it and outside the range
    dets[0, 8, :3] = (6.0, 3.2, -1.0)                                       # straddles the left border: clipped
    count = [40, 33]
    c = kc.kitti_rows(dets, count, cal.lidar2cam, cal.p2, cal.image_shape, limit, lidar_input)
    assert not c["open"].any() and c["rows32"].dtype == np.float32
    names = ["Car", "Pedestrian", "Cyclist"]
    got = kitti_eval.rows_to_annos(c["rows32"], c["src"], c["count"], dets, names, [100, 101])
    want = _host_annos(dets, count, cal, limit, lidar_input, names)
    compare_annos(got, want, host_bounds(dets, c, cal), f"{limit} {lidar_input}")
    n_dropped = 73 - int(c["count"].sum())
    assert n_dropped == {(True, False): 5, (False, False): 2, (True, True): 4}[(limit is not None, lidar_input)]
    if not lidar_input:
        row = int(np.flatnonzero(c["src"][0] == 8)[0])
        assert c["rows"][0, row, 1] == 0.0 and c["rows"][0, row, 3] > 0       # the straddling box is kept with x1 clipped to 0
    lines = kitti_eval.kitti_result_lines(got[0])
    assert len(lines) == c["count"][0] and lines[0].split()[0] in names and len(lines[0].split()) == 16


def test_contract_rows_special_rows():
    """count 0 and above M, a NaN row (compares false everywhere: kept, NaN through), a box behind the camera, the empty annotation"""
    cal = calibration((0, 1))
    dets = detections(6, 2, 5, cal)
    dets[1, 1, 0] = np.nan
    dets[1, 2, :2] = (-20.0, 1.0)                                           # behind the camera: outside the range, and its image box is the mirror's
    c = kc.kitti_rows(dets, [0, 9], cal.lidar2cam, cal.p2, cal.image_shape, CAR_RANGE, False)
    assert c["count"].tolist() == [0, 4] and c["src"][1].tolist() == [0, 1, 3, 4, -1] and (c["src"][0] == -1).all() and not c["rows"][0].any()
    assert np.isnan(c["rows"][1, 1, [0, 1, 2, 3, 4, 8]]).all() and c["rows"][1, 1, 12] == dets[1, 1, 7]
    annos = kitti_eval.rows_to_annos(c["rows32"], c["src"], c["count"], dets, ["Car", "Pedestrian", "Cyclist"], [7, 8])
    assert set(annos[0]) == set(kitti_eval.empty_result_anno()) | {"image_idx"} and annos[0]["bbox"].shape == (0, 4) and annos[1]["image_idx"].tolist() == [8] * 4
    free = kc.kitti_rows(dets, [5, 5], cal.lidar2cam, cal.p2, cal.image_shape, None, True)
    assert free["count"].tolist() == [5, 5]                                 # both filters off: everything is reported


def test_configs_load_and_build_their_ops():
    from minddet.models import Config, build_detector

    car = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", "pointpillars_car_xyres16_kitti.py"))
    base = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", "pointpillars_car_xyres16_points.py"))
    assert dict(car.model) == dict(base.model)
    extra = {k: v for k, v in dict(car.test_cfg).items() if k not in base.test_cfg or base.test_cfg[k] != v}
    assert extra == dict(remove_outside_points=True, lidar_input=False) and car.test_cfg["post_center_limit_range"] == CAR_RANGE
    tiny = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", "pointpillars_tiny_kitti.py"))
    tbase = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", "pointpillars_tiny_points.py"))
    assert dict(tiny.model) == dict(tbase.model) and tiny.test_cfg["remove_outside_points"] is True
    det = build_detector(dict(tiny.model), None, tiny.test_cfg)
    assert det._kitti_options() == (True, False, [1.6, -2.56, -4.5, 7.68, 2.56, 2.5]) and callable(det.prepare_kitti) and callable(det.forward_kitti)
    for bad in (dict(remove_environment=True), dict(random_crop=True), dict(use_self_train=False), dict(fp32_calibration=True)):
        with pytest.raises(ValueError):
            build_detector(dict(tiny.model), None, dict(tiny.test_cfg, **bad))._kitti_options()
    assert build_detector(dict(tiny.model), None, dict(tiny.test_cfg, remove_environment=False, use_self_train=True))._kitti_options()[0] is True


def test_refused_options_raise():
    z = fixture()
    args = [z[f"cal0_{k}"] for k in ("rect", "trv2c", "p2", "image_shape")]
    for kw in (dict(remove_environment=True), dict(random_crop=True), dict(generate_single_sample_dict=True), dict(use_self_train=False),
               dict(fp32_calibration=True), dict(no_such_option=1)):
        with pytest.raises(ValueError):
            det_ops.KittiCalibration(*args, device="cpu", **kw)
    assert det_ops.KittiCalibration(*args, device="cpu", remove_environment=False, random_crop=None, use_self_train=True).B == 1
    with pytest.raises(ValueError):                           # KITTI's 3x4 not extended
        det_ops.KittiCalibration(args[0], args[1], args[2][:3], args[3], device="cpu")
    with pytest.raises(ValueError):
        det_ops.KittiCalibration(args[0], args[1], args[2], [375, 1242, 3], device="cpu")
    cal = calibration((0,))
    with pytest.raises(ValueError):
        cal.detection_frustums_host(np.zeros((1, det_ops.CROP_MAX_HULLS + 1, 4)))
    with pytest.raises(ValueError):
        cal.detection_frustums_host(np.zeros((2, 3, 4)))
    # the operand checks of the thin wrappers come before any device call
    hulls, cnt, offs = torch.zeros((1, 2, 8, 3), dtype=torch.float64), torch.zeros((1,), dtype=torch.int32), torch.zeros((2,), dtype=torch.int32)
    for bad in (torch.zeros((4, 3)), torch.zeros((4, 5)), torch.zeros((4,))):      # F != 4
        with pytest.raises(ValueError):
            det_ops.crop_hulls(bad, offs, hulls, cnt)
    for args in ((offs, hulls[:, :, :7], cnt), (offs, hulls, torch.zeros((2,), dtype=torch.int32)), (offs[:1], hulls, cnt),
                 (offs, torch.zeros((1, 65, 8, 3), dtype=torch.float64), cnt)):
        with pytest.raises(ValueError):
            det_ops.crop_hulls(torch.zeros((4, 4)), *args)
    with pytest.raises(ValueError):
        det_ops.crop_hulls(torch.zeros((4, 4)), offs, hulls, cnt, out=torch.zeros((3, 4)))
    eye = torch.eye(4, dtype=torch.float64)[None]
    with pytest.raises(ValueError):
        det_ops.kitti_boxes_to_lidar(torch.zeros((1, 3, 6)), cnt, eye)
    with pytest.raises(ValueError):
        det_ops.kitti_boxes_to_lidar(torch.zeros((1, 3, 7)), cnt, eye[0])
    shape = torch.zeros((1, 2), dtype=torch.int32)
    for args, kw in (((torch.zeros((1, 3, 8)), cnt, eye, eye, shape), {}), ((torch.zeros((1, 513, 9)), cnt, eye, eye, shape), {}),
                     ((torch.zeros((1, 3, 9)), cnt, eye, eye[0], shape), {}), ((torch.zeros((1, 3, 9)), cnt, eye, eye, shape[0]), {}),
                     ((torch.zeros((1, 3, 9)), cnt, eye, eye, shape), dict(limit_range=[0, 1, 2])),
                     ((torch.zeros((1, 3, 9)), cnt, eye, eye, shape), dict(limit_range=[0, 0, 0, 1, 1, float("nan")]))):
        with pytest.raises(ValueError):
            det_ops.kitti_rows(*args, **kw)
    for kw in (dict(remove_outside_points=True), dict(reference_detections=True), dict(remove_environment=True)):      # PointCloudAugment keeps refusing what it refused
        with pytest.raises(ValueError):
            det_ops.PointCloudAugment((0, -40, 70, 40), **kw)
