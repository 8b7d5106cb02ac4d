"""CPU: the KITTI AP evaluation operators without a GPU -- the ABI of include/minddet_hip_kittieval.h (the five functions exported, header
and Makefile wired, every documented rc 2 / rc 4 and aliasing answered before any device call, the ctypes
mirrors and limits laid out as the header says), kitti_eval.pack_annos' codes against what clean_data derives from the names, the
Python layer's refusals, and eval_class after its tail moved into the helper eval_class_device shares."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from minddet_amd import _lib, det_ops
from minddet_amd import kitti_eval as ke
from tests import abi_header as ah
from tests.abi_cases_kittieval import CASES, CN, DT, GT, K, NI, PTS, FlagsAttrs, OverlapsAttrs, StatsAttrs
from tests.abi_derive import attr, edited, lib_handle, rc, refuse_single_defects, shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["md_kitti_eval_flags", "md_kitti_eval_overlaps", "md_kitti_eval_match", "md_kitti_eval_thresholds", "md_kitti_eval_stats"]
ARG, SIZE = 2, 4
BY_ID = {c.id: c for c in CASES}


def _golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "kitti_eval_vectors.json")))


def _np_anno(a):
    return {k: (np.array(v) if k == "name" else np.asarray(v, float if k != "occluded" else int)) for k, v in a.items()}


def test_header_declares_the_symbols_and_the_library_exports_them():
    hdr = ah.header("minddet_hip_kittieval.h")
    assert ah.aot_symbols(hdr) == SYMS and "_workspace_bytes" not in hdr
    for cite in ("eval_gpu/eval.py:9-27", "eval_utils.py:36-115", "rotate_iou.py:167-302", "ground-truth-major"):
        assert cite in hdr, cite
    mk = open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    assert "minddet_hip_kittieval.h" in mk
    src = open(os.path.join(ROOT, "minddet_amd", "csrc", "kittieval.hip")).read()
    assert src.index("#pragma clang fp contract(off)") < src.index('#include "aot.h"') and ".acquire(" not in src and not re.search(r"atomic\w*\(", src)
    assert {c.sym for c in CASES} == set(SYMS) and len({c.id for c in CASES}) == len(CASES)
    lib = lib_handle()
    for sym in SYMS:
        assert getattr(lib, sym)(0, None, None, None, None, None, None) == 1      # wrong parameter count, before anything else
        assert sym not in _lib.exported_symbols()                                  # declared in the new header only
    for other in ("minddet_hip.h", "minddet_hip_kitti.h"):
        assert "md_kitti_eval" not in open(os.path.join(ROOT, "include", other)).read()
    # the pair arithmetic has one home, and both kernels call it
    csrc = os.path.join(ROOT, "minddet_amd", "csrc")
    assert "rie_pair(" in open(os.path.join(csrc, "nms.hip")).read() and "rie_pair(" in src
    assert "rie_in_quad" not in open(os.path.join(csrc, "nms.hip")).read() and "rie_in_quad" in open(os.path.join(csrc, "rot_eval.h")).read()


def test_ctypes_mirrors_and_limits_have_the_headers_layout():
    hdr = ah.header("minddet_hip_kittieval.h")

    def fields(name):
        return ah.statements(name, hdr)

    assert fields("md_kitti_eval_flags_attrs") == ["int32_t abs_gt_height"]
    assert fields("md_kitti_eval_overlaps_attrs") == ["int32_t metric"]
    assert fields("md_kitti_eval_stats_attrs") == ["int32_t metric", "int32_t compute_aos"]
    for got in (det_ops._KittiEvalFlagsAttrs, FlagsAttrs):
        assert C.sizeof(got) == 4 and got.abs_gt_height.offset == 0
    for got in (det_ops._KittiEvalOverlapsAttrs, OverlapsAttrs):
        assert C.sizeof(got) == 4 and got.metric.offset == 0
    for got in (det_ops._KittiEvalStatsAttrs, StatsAttrs):
        assert C.sizeof(got) == 8 and got.metric.offset == 0 and got.compute_aos.offset == 4
    for name, macro, ke_name in (("KEVAL_MAX_DETS", "MD_KEVAL_MAX_DETS", "MAX_DETS"), ("KEVAL_MAX_GTS", "MD_KEVAL_MAX_GTS", "MAX_GTS"),
                                 ("KEVAL_MAX_IMAGES", "MD_KEVAL_MAX_IMAGES", "MAX_IMAGES"), ("KEVAL_MAX_CLASSES", "MD_KEVAL_MAX_CLASSES", "MAX_CLASSES"),
                                 ("KEVAL_MAX_LEVELS", "MD_KEVAL_MAX_LEVELS", "MAX_LEVELS"), ("KEVAL_SAMPLE_PTS", "MD_KEVAL_SAMPLE_PTS", "N_SAMPLE_PTS")):
        assert getattr(det_ops, name) == getattr(ke, ke_name) == ah.defines(hdr)[macro]
    assert det_ops.KEVAL_MAX_DETS == det_ops.KITTI_MAX_DETS == 512 and det_ops.KEVAL_SAMPLE_PTS == PTS == 41


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_kittieval", case)


def _described(case, shapes):
    """the call of `case` with the shapes of some operands replaced in the description alone (the host blocks stay small: a refused
    call touches nothing)"""
    call = edited(case, lambda c: None)
    for i, shp in shapes.items():
        call.shapes[i] = list(shp)
    return call.run(lib_handle())


def test_semantic_refusals_return_the_documented_codes():
    flags, ov0, ov1 = BY_ID["md_kitti_eval_flags[full]"], BY_ID["md_kitti_eval_overlaps[metric 0]"], BY_ID["md_kitti_eval_overlaps[metric 1]"]
    match, thr, stats = BY_ID["md_kitti_eval_match"], BY_ID["md_kitti_eval_thresholds"], BY_ID["md_kitti_eval_stats[metric 0, aos 1]"]
    # every extent that disagrees: rc 2
    for i, e in enumerate([shape(0, (GT, 3)), shape(0, (GT + 1, 4)), shape(1, (GT - 1,)), shape(2, (GT + 1,)), shape(3, (CN, GT + 1)), shape(4, (DT, 5)),
                           shape(5, (CN + 1, DT)), shape(5, (CN, DT - 1)), shape(6, (CN, 2, GT)), shape(6, (CN, 3, GT + 1)), shape(7, (CN + 1, 3, DT)),
                           shape(7, (CN, 3, DT + 1)), shape(8, (CN, 2)), shape(8, (CN + 1, 3)), attr("abs_gt_height", 2), attr("abs_gt_height", -1)]):
        assert rc(flags, e) == ARG, i
    for i, e in enumerate([shape(1, (NI,)), shape(2, (NI + 2,)), shape(3, (GT, 7)), shape(4, (DT, 7)), shape(3, (GT, 5)), attr("metric", 3), attr("metric", -1)]):
        assert rc(ov0, e) == ARG, i
    for i, e in enumerate([shape(3, (GT, 4)), shape(4, (DT, 4)), shape(4, (DT, 5))]):
        assert rc(ov1, e) == ARG, i
    common = [shape(1, (CN, 2, GT)), shape(2, (CN + 1, 3, DT)), shape(2, (CN, 2, DT)), shape(3, (DT + 1,)), shape(5, (NI,)), shape(6, (NI + 2,)),
              shape(7, (CN + 1, K))]
    for i, e in enumerate(common + [shape(8, (CN, 3, K, GT + 1)), shape(8, (CN, 3, K + 1, GT)), shape(8, (CN, 2, K, GT)), shape(8, (CN + 1, 3, K, GT))]):
        assert rc(match, e) == ARG, i
    for i, e in enumerate([shape(0, (CN, 2, K, GT)), shape(1, (CN, 2)), shape(1, (CN + 1, 3)), shape(2, (CN, 3, K, PTS - 1)), shape(2, (CN, 3, K + 1, PTS)),
                           shape(3, (CN, 3, K + 1)), shape(3, (CN + 1, 3, K))]):
        assert rc(thr, e) == ARG, i
    for i, e in enumerate(common + [shape(8, (CN, 3, K, PTS + 1)), shape(9, (CN, 3, K + 1)), shape(10, (GT, 5)), shape(10, (GT + 1, 4)), shape(11, (GT + 1,)),
                                    shape(12, (DT - 1, 4)), shape(13, (GT + 1,)), shape(14, (DT + 1,)), shape(15, (CN, 3, K, PTS, NI, 2)),
                                    shape(15, (CN, 3, K, PTS, NI + 1, 3)), shape(16, (CN, 3, K, PTS, NI + 1)), shape(17, (CN, 3, K, PTS, 4)),
                                    shape(17, (CN, 3, K + 1, PTS, 3)), shape(18, (CN, 3, K, PTS - 1)), attr("metric", 3), attr("metric", -1),
                                    attr("compute_aos", 2), attr("compute_aos", -1)]):
        assert rc(stats, e) == ARG, i
    # every documented limit: rc 4 (the descriptions alone say so)
    C1, K1, I1 = det_ops.KEVAL_MAX_CLASSES + 1, det_ops.KEVAL_MAX_LEVELS + 1, det_ops.KEVAL_MAX_IMAGES + 1
    G1, D1 = det_ops.KEVAL_MAX_IMAGES * det_ops.KEVAL_MAX_GTS + 1, det_ops.KEVAL_MAX_IMAGES * det_ops.KEVAL_MAX_DETS + 1
    assert _described(flags, {3: (C1, GT), 5: (C1, DT), 6: (C1, 3, GT), 7: (C1, 3, DT), 8: (C1, 3)}) == SIZE
    assert _described(flags, {0: (G1, 4), 1: (G1,), 2: (G1,), 3: (CN, G1), 6: (CN, 3, G1)}) == SIZE
    assert _described(flags, {4: (D1, 4), 5: (CN, D1), 7: (CN, 3, D1)}) == SIZE
    assert _described(ov0, {0: (I1 + 1,), 1: (I1 + 1,), 2: (I1 + 1,)}) == SIZE
    assert _described(ov0, {5: (1 << 31,)}) == SIZE and _described(ov1, {3: (G1, 7)}) == SIZE and _described(ov1, {4: (D1, 7)}) == SIZE
    assert _described(match, {0: (1 << 31,)}) == SIZE
    assert _described(match, {4: (I1 + 1,), 5: (I1 + 1,), 6: (I1 + 1,)}) == SIZE
    assert _described(match, {7: (CN, K1), 8: (CN, 3, K1, GT)}) == SIZE
    assert _described(match, {1: (C1, 3, GT), 2: (C1, 3, DT), 7: (C1, K), 8: (C1, 3, K, GT)}) == SIZE
    assert _described(match, {1: (CN, 3, G1), 8: (CN, 3, K, G1)}) == SIZE and _described(match, {2: (CN, 3, D1), 3: (D1,)}) == SIZE
    assert _described(thr, {0: (C1, 3, K, GT), 1: (C1, 3), 2: (C1, 3, K, PTS), 3: (C1, 3, K)}) == SIZE
    assert _described(thr, {0: (CN, 3, K1, GT), 2: (CN, 3, K1, PTS), 3: (CN, 3, K1)}) == SIZE and _described(thr, {0: (CN, 3, K, G1)}) == SIZE
    assert _described(stats, {0: (1 << 31,)}) == SIZE
    assert _described(stats, {4: (I1 + 1,), 5: (I1 + 1,), 6: (I1 + 1,), 15: (CN, 3, K, PTS, I1, 3), 16: (CN, 3, K, PTS, I1)}) == SIZE
    assert _described(stats, {7: (CN, K1), 8: (CN, 3, K1, PTS), 9: (CN, 3, K1), 15: (CN, 3, K1, PTS, NI, 3), 16: (CN, 3, K1, PTS, NI), 17: (CN, 3, K1, PTS, 3),
                              18: (CN, 3, K1, PTS)}) == SIZE
    assert _described(stats, {2: (CN, 3, D1), 3: (D1,), 12: (D1, 4), 14: (D1,)}) == SIZE


def test_aliased_outputs_are_refused():
    """an output at the address of an input or of another output: rc 2 before any device call"""
    lib = lib_handle()
    for cid, pairs in (("md_kitti_eval_flags[full]", ((6, 3), (7, 5), (7, 6), (8, 1))), ("md_kitti_eval_overlaps[metric 0]", ((5, 3), (5, 4))),
                       ("md_kitti_eval_match", ((8, 0), (8, 3))), ("md_kitti_eval_thresholds", ((2, 0), (3, 1), (3, 2))),
                       ("md_kitti_eval_stats[metric 0, aos 1]", ((15, 9), (16, 0), (17, 15), (18, 16), (18, 8)))):
        case = BY_ID[cid]
        for out, other in pairs:
            n, ops = len(case.operands), case.operands
            bufs = [(C.c_char * 65536)() for _ in range(n)]
            params = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
            params[out] = params[other]
            ndims = (C.c_int * n)(*[len(t.shape) for t in ops])
            keep = [(C.c_int64 * max(len(t.shape), 1))(*t.shape) for t in ops]
            shapes = (C.POINTER(C.c_int64) * n)(*[C.cast(k, C.POINTER(C.c_int64)) for k in keep])
            dtypes = (C.c_char_p * n)(*[t.dtype.encode() for t in ops])
            assert getattr(lib, case.sym)(n, params, ndims, shapes, dtypes, None, C.byref(case.extra) if case.extra is not None else None) == 2, (cid, out, other)


@pytest.mark.parametrize("table", [ke.CLASS_NAMES_FULL, ke.CLASS_NAMES_MS], ids=["full", "ms"])
def test_pack_annos_codes_equal_what_clean_data_derives_from_the_names(table):
    case = _golden()["cases"][0]
    gt, dt = [_np_anno(a) for a in case["gt"]], [_np_anno(a) for a in case["dt"]]
    p = ke.pack_annos(gt, dt, table, device="cpu")
    assert p.I == len(gt) == 50 and p.gt_cam is None and p.dt_cam is None and p.abs_gt_height == (table is ke.CLASS_NAMES_MS)
    g_off, d_off, o_off = p.gt_off.numpy(), p.dt_off.numpy(), p.ov_off.numpy()
    assert p.gt_off.dtype == p.dt_off.dtype == torch.int32 and p.ov_off.dtype == torch.int64 and p.gt_valid.shape == (len(table), g_off[-1])
    assert p.gt_box.dtype == p.dt_score.dtype == torch.float64 and p.gt_occ.dtype == torch.int32 and p.gt_dc.dtype == p.dt_same.dtype == torch.uint8
    for i, (g, d) in enumerate(zip(gt, dt)):
        G, D = len(g["name"]), len(d["name"])
        assert g_off[i + 1] - g_off[i] == G and d_off[i + 1] - d_off[i] == D and o_off[i + 1] - o_off[i] == G * D
        assert np.array_equal(p.gt_box[g_off[i]:g_off[i + 1]].numpy(), g["bbox"].reshape(-1, 4)) and np.array_equal(p.dt_score[d_off[i]:d_off[i + 1]].numpy(), d["score"])
        # clean_data on a copy whose boxes are tall and unoccluded leaves the name rules alone: counted = the class, ignored = its neighbour
        tall = lambda a: dict(a, bbox=np.tile([0.0, 0.0, 100.0, 100.0], (len(a["name"]), 1)), occluded=np.zeros(len(a["name"]), int),
                              truncated=np.zeros(len(a["name"])))
        for c in range(len(table)):
            _, ig, idt, dc = ke.clean_data(tall(g), tall(d), c, 0, table)
            assert (p.gt_valid[c, g_off[i]:g_off[i + 1]].numpy().astype(int) - 1).tolist() == [{0: 1, 1: 0, -1: -1}[f] for f in ig], (i, c)
            assert p.dt_same[c, d_off[i]:d_off[i + 1]].numpy().tolist() == [int(f == 0) for f in idt], (i, c)
            assert int(p.gt_dc[g_off[i]:g_off[i + 1]].sum()) == len(dc)
    assert p.pairs == o_off[-1] and int(p.gt_dc.sum()) > 0 and int((p.gt_valid == 1).sum()) > 0
    if table is ke.CLASS_NAMES_MS:
        assert torch.equal(p.gt_valid[0], p.gt_valid[5])                      # the duplicate "car" follows the table by index


def test_python_layer_refuses_before_any_device_call():
    case = _golden()["cases"][0]
    gt, dt = [_np_anno(a) for a in case["gt"]], [_np_anno(a) for a in case["dt"]]
    p = ke.pack_annos(gt, dt, device="cpu")
    mo = np.full((2, 3, 1), 0.5)
    for metric in (1, 2):                                                     # the fixture's detections carry no location / dimensions / rotation_y
        with pytest.raises(ValueError):
            ke.eval_class_device(p, [0], [0, 1, 2], metric, mo)
    with pytest.raises(ValueError):
        ke.eval_class_device(p, [0], [0, 1, 2], 3, mo)
    with pytest.raises(ValueError):
        ke.eval_class_device(p, [0, 1], [0], 0, mo)                           # min_overlaps has one class column
    with pytest.raises(ValueError):
        ke.eval_class_device(p, [6], [0], 0, mo)
    with pytest.raises(ValueError):
        ke.eval_class_device(p, [0], [0], 0, np.full((5, 3, 1), 0.5))         # K > 4
    with pytest.raises(ValueError):
        ke.eval_class_device(ke.pack_annos(gt, None, device="cpu"), [0], [0], 0, mo)
    with pytest.raises(ValueError):
        ke.pack_annos(gt, dt[:-1], device="cpu")
    with pytest.raises(ValueError):
        ke.pack_annos(gt, dt, ["a"] * 9, device="cpu")
    big = dict(gt[0], name=np.array(["Car"] * 513), bbox=np.zeros((513, 4)), alpha=np.zeros(513), occluded=np.zeros(513, int), truncated=np.zeros(513))
    with pytest.raises(ValueError):
        ke.pack_annos([big], [dt[0]], device="cpu")
    bigd = dict(dt[0], name=np.array(["Car"] * 513), bbox=np.zeros((513, 4)), alpha=np.zeros(513), score=np.zeros(513))
    with pytest.raises(ValueError):
        ke.pack_annos([gt[0]], [bigd], device="cpu")
    with pytest.raises(ValueError):
        ke.get_official_eval_result(gt, dt, [0], protocol="ms", backend="numpy")
    with pytest.raises(ValueError):
        ke.get_official_eval_result(gt, dt, [0], protocol="ms", packed=p)      # a pack is the device backend's
    with pytest.raises(ValueError):
        ke.get_official_eval_result(gt, dt, [0], protocol="ms", backend="device", packed=p)      # packed with the other class table
    with pytest.raises(ValueError):
        p.with_rows(torch.zeros((49, 4, 14)), torch.zeros((49,), dtype=torch.int32), ["Car"])
    with pytest.raises(ValueError):
        p.with_rows(torch.zeros((50, 513, 14)), torch.zeros((50,), dtype=torch.int32), ["Car"])
    # the thin wrappers check shapes and limits first
    f64, u8, i32t = torch.float64, torch.uint8, torch.int32
    z = lambda *s, dtype=f64: torch.zeros(s, dtype=dtype)
    for args in ((z(5, 3), z(5, dtype=i32t), z(5), z(2, 5, dtype=u8), z(6, 4), z(2, 6, dtype=u8)), (z(5, 4), z(4, dtype=i32t), z(5), z(2, 5, dtype=u8), z(6, 4), z(2, 6, dtype=u8)),
                 (z(5, 4), z(5, dtype=i32t), z(5), z(9, 5, dtype=u8), z(6, 4), z(9, 6, dtype=u8)), (z(5, 4), z(5, dtype=i32t), z(5), z(2, 5, dtype=u8), z(6, 4), z(3, 6, dtype=u8))):
        with pytest.raises(ValueError):
            det_ops.kitti_eval_flags(*args)
    off, off64 = z(3, dtype=i32t), z(3, dtype=torch.int64)
    for args in ((off, off, off64, z(5, 4), z(6, 4), 3, 16), (off, off, off64, z(5, 4), z(6, 4), 1, 16), (off, off[:2], off64, z(5, 4), z(6, 4), 0, 16),
                 (off, off, off64, z(5, 4), z(6, 4), 0, 1 << 31)):
        with pytest.raises(ValueError):
            det_ops.kitti_eval_overlaps(*args)
    m = (z(16), z(2, 3, 5, dtype=u8), z(2, 3, 6, dtype=u8), z(6), off, off, off64, z(2, 2))
    for i, bad in ((1, z(2, 2, 5, dtype=u8)), (2, z(3, 3, 6, dtype=u8)), (3, z(7)), (5, off[:2]), (7, z(3, 2)), (7, z(2, 5))):
        with pytest.raises(ValueError):
            det_ops.kitti_eval_match(*[bad if j == i else t for j, t in enumerate(m)])
    with pytest.raises(ValueError):
        det_ops.kitti_eval_thresholds(z(2, 3, 2, 5), z(3, 3, dtype=i32t))
    with pytest.raises(ValueError):
        det_ops.kitti_eval_thresholds(z(2, 3, 5, 5), z(2, 3, dtype=i32t))
    rest = (z(2, 3, 2, 41), z(2, 3, 2, dtype=i32t), z(5, 4), z(5, dtype=u8), z(6, 4), z(5), z(6))
    for i, bad in ((0, z(2, 3, 2, 40)), (1, z(2, 3, 3, dtype=i32t)), (2, z(5, 5)), (3, z(4, dtype=u8)), (4, z(5, 4)), (5, z(6)), (6, z(5))):
        with pytest.raises(ValueError):
            det_ops.kitti_eval_stats(*m, *[bad if j == i else t for j, t in enumerate(rest)], 0)
    with pytest.raises(ValueError):
        det_ops.kitti_eval_stats(*m, *rest, 3)


def test_eval_class_still_gives_the_fixtures_rows():
    """the tail of eval_class now lives in _curves_from_counts: the reference's own precision rows, NaN as -1, to 1e-12 as before"""
    mo = np.array([[[0.7, 0.5, 0.5]] * 3, [[0.5, 0.25, 0.25]] * 3])
    for case in _golden()["cases"]:
        gt, dt = [_np_anno(a) for a in case["gt"]], [_np_anno(a) for a in case["dt"]]
        ret = ke.eval_class(gt, dt, [0, 1, 2], [0, 1, 2], 0, mo, class_names=ke.CLASS_NAMES_MS)
        np.testing.assert_allclose(np.nan_to_num(ret["precision"], nan=-1.0), np.array(case["precision"]), rtol=0, atol=1e-12)
    # the helper on a hand-made table: the divisions, then the right-to-left maximum over the whole row
    pr = np.array([[1, 0, 3, 0.9], [2, 2, 2, 1.5], [1, 3, 3, 0.2], [3, 1, 1, 2.0]], float)
    prec, rec, aos = np.zeros(41), np.zeros(41), np.zeros(41)
    ke._curves_from_counts(pr, prec, rec, aos)
    assert prec[:4].tolist() == [1.0, 0.75, 0.75, 0.75] and not prec[4:].any()
    assert rec[:4].tolist() == [0.75, 0.75, 0.75, 0.75] and aos[:4].tolist() == [0.9, 0.5, 0.5, 0.5]
