"""CPU: the CenterPoint post-processing chain without a GPU -- the ABI of include/minddet_hip_cp.h (every declared function exported, the ctypes mirrors of the two attribute structs laid out
as the header says), the semantic refusals, the tiny config, and the one statement of the per-cell arithmetic."""
import ctypes as C
import os

import pytest

from minddet_amd import det_ops, graphs
from tests import abi_header as ah
from tests.abi_cases import I
from tests.abi_cases_cp import CASES, CPHead, NmsRotated
from tests.abi_derive import attr, lib_handle, rc, refuse_single_defects, shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = ah.header("minddet_hip_cp.h")
SYMS = ["md_nms_rotated", "md_cp_scores", "md_cp_decode_selected", "md_cp_pack"]


def test_header_declares_the_four_symbols_and_the_library_exports_them():
    main = ah.header("minddet_hip.h")
    assert ah.aot_symbols(HDR) == SYMS and '#include "minddet_hip.h"' in HDR
    assert not set(SYMS) & set(ah.aot_symbols(main))
    assert {c.sym for c in CASES} == set(SYMS) and len({c.id for c in CASES}) == len(CASES)
    assert "minddet_hip_cp.h" in open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    lib = lib_handle()
    for n in SYMS:
        assert hasattr(lib, n), n
        assert getattr(lib, n)(0, None, None, None, None, None, None) == 1      # wrong parameter count, before anything else


def test_ctypes_mirrors_have_the_headers_layout():
    task = ah.struct_of("md_cp_task_attrs", HDR)
    head = ah.struct_of("md_cp_head_attrs", HDR, known={"md_cp_task_attrs": task})
    nms = ah.struct_of("md_nms_rotated_attrs", HDR)
    assert C.sizeof(task) == 32 and C.sizeof(head) == 4 + 8 * 32 + 12 * 4 + 4 and C.sizeof(nms) == 12
    for want, mirrors in ((head, (det_ops._CPHeadAttrs, CPHead)), (nms, (det_ops._NmsRotatedAttrs, NmsRotated)),
                          (task, (det_ops._CPTaskAttrs,))):
        for got in mirrors:
            assert ah.same_layout(got, want), got
    assert dict(det_ops._CPHeadAttrs._fields_)["task"]._type_ is det_ops._CPTaskAttrs and det_ops.CP_MAX_TASKS == 8


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_cp", case)


def test_semantic_refusals_return_the_documented_codes():
    by = {c.id: c for c in CASES}
    ARG, SIZE = 2, 4

    def task(t, name, value):
        return lambda c: setattr(c.extra.task[t], name, value)

    nms = by["md_nms_rotated[count]"]
    for e in (attr("mode", 2), attr("mode", -1), attr("max_output", -1), shape(0, (2, 4, 6)), shape(1, (3,), I), shape(2, (2, 5), I),
              shape(3, (3,), I)):
        assert rc(nms, e) == ARG
    for e in (shape(0, (2, 65537, 7)), shape(0, (65536, 1, 7))):
        assert rc(nms, e) == SIZE
    sc, dec, pack = by["md_cp_scores"], by["md_cp_decode_selected"], by["md_cp_pack"]
    head_edits = (attr("num_tasks", 0), attr("num_tasks", 9), task(0, "num_classes", 0), task(1, "off_hm", 23), task(1, "off_hm", -1),
                  task(0, "off_vel", -2), task(0, "off_vel", 23), task(1, "off_dim", 22), task(0, "off_reg", -1), task(1, "off_rot", 23),
                  task(0, "off_height", 24))
    for e in head_edits + (shape(1, (1, 3, 16)), shape(1, (1, 2, 15)), shape(1, (2, 2, 16))):
        assert rc(sc, e) == ARG
    assert rc(sc, shape(0, (1, 4, 4, 488), "bfloat16")) == SIZE
    for e in head_edits + (shape(1, (1, 3, 3), I), shape(1, (2, 2, 3), I), shape(2, (1, 3), I), shape(3, (1, 2, 3, 8)), shape(3, (1, 2, 4, 9)),
                           shape(4, (1, 2, 3, 9)), shape(5, (1, 2, 4), I)):
        assert rc(dec, e) == ARG
    for e in (attr("num_tasks", 3), attr("num_tasks", 0), attr("max_per_task", -1), attr("max_per_task", 3), shape(0, (1, 2, 3, 8)),
              shape(1, (1, 2, 4)), shape(2, (1, 3, 3), I), shape(3, (2, 2, 3), I), shape(4, (1, 3), I), shape(5, (2, 2), I), shape(6, (1, 4, 10)),
              shape(6, (1, 5, 11)), shape(7, (2,), I)):
        assert rc(pack, e) == ARG


def test_tiny_config_and_the_switch():
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_tiny.py"))
    nusc = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc.py"))
    assert cfg.model == nusc.model and cfg.data["pseudo_image_hw"] == (128, 128)
    assert (cfg.test_cfg["nms"]["nms_pre_max_size"], cfg.test_cfg["nms"]["nms_post_max_size"]) == (256, 20)
    m = build_detector(dict(cfg.model, seed=3), cfg.train_cfg, cfg.test_cfg)
    assert type(m) is graphs.PointPillars and m.cp_post == graphs.CP_POST and m.bbox_head.num_classes == [1, 2, 2, 1, 2, 2]
    assert graphs.CP_POST == (os.environ.get("MD_CP_POST", "0") == "1")
    for v in (True, False):
        assert build_detector(dict(cfg.model, seed=3, cp_post=v), cfg.train_cfg, cfg.test_cfg).cp_post is v
    at = m.post_batched().at
    assert at.num_tasks == 6 and at.max_per_task == 20 and [at.task[t].class_base for t in range(6)] == [0, 1, 3, 5, 6, 8]
    assert [at.task[t].off_hm for t in range(6)] == [o["hm"] for o in m.bbox_head.task_offsets()]
    with pytest.raises(ValueError):
        det_ops.cp_head_attrs([dict(reg=0, height=2, dim=3, rot=6, hm=8)] * 9, [1] * 9, cfg.test_cfg)


def test_cell_arithmetic_is_stated_once():
    src = {n: open(os.path.join(ROOT, "minddet_amd", "csrc", n)).read() for n in ("detops.hip", "cphead.hip", "box_codec.h", "nms.hip")}
    for n in ("detops.hip", "cphead.hip"):
        assert '#include "box_codec.h"' in src[n] and "cp_score_one(" in src[n] and "cp_box_one(" in src[n], n
        assert "atan2f(" not in src[n]                                         # no second statement of the decode
    assert "atan2f(" in src["box_codec.h"]
    # one statement of the rotated suppression predicate for the single-list and the batched kernel
    assert src["nms.hip"].count("rot_overlap(A, col, scratch, 256)") == 1 and src["nms.hip"].count("rot_mask_tile<MODE>(") == 2
