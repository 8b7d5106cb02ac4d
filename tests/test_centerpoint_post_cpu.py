"""CPU: the CenterPoint post-processing chain without a GPU -- the ABI of include/minddet_hip_cp.h (every declared function exported, the
single-defect calls refused with the documented codes before any device call, the ctypes mirrors of the two attribute structs laid out
as the header says), the semantic refusals, the tiny config, and the one statement of the per-cell arithmetic."""
import copy
import ctypes as C
import os
import re

import pytest

from minddet_amd import _lib, det_ops, graphs
from tests.abi_cases import F, I, T
from tests.abi_cases_cp import CASES, CPHead, NmsRotated
from tests.test_abi_checks_cpu import Call, mutations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "minddet_hip_cp.h")).read()
SYMS = ["md_nms_rotated", "md_cp_scores", "md_cp_decode_selected", "md_cp_pack"]
CTYPE = {"int32_t": C.c_int32, "float": C.c_float}


def _lib_handle():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return C.CDLL(_lib.LIB_PATH)


def _struct_fields(name, known):
    """[(field, ctypes type)] of `typedef struct name { ... } name;` in the header: int32_t / float scalars and arrays, arrays of an
    earlier struct (`known`), extents given as numbers or as a #define of the header"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HDR, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    defines = {k: int(v) for k, v in re.findall(r"^#define (\w+) (\d+)\s*$", HDR, flags=re.M)}
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        ty, rest = stmt.split(None, 1)
        base = CTYPE.get(ty) or known[ty]
        for decl in rest.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[(\w+)\])?\s*", decl)
            ext = m.group(2)
            out.append((m.group(1), base if ext is None else base * (defines[ext] if ext in defines else int(ext))))
    return out


def test_header_declares_the_four_symbols_and_the_library_exports_them():
    main = open(os.path.join(ROOT, "include", "minddet_hip.h")).read()
    pat = r"^\s*int\s+(\w+)\s*\(MD_AOT_ARGS\)\s*;"
    assert re.findall(pat, HDR, flags=re.M) == SYMS and '#include "minddet_hip.h"' in HDR
    assert not set(SYMS) & set(re.findall(pat, main, flags=re.M))
    assert {c.sym for c in CASES} == set(SYMS) and len({c.id for c in CASES}) == len(CASES)
    assert "minddet_hip_cp.h" in open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    lib = _lib_handle()
    for n in SYMS:
        assert hasattr(lib, n), n
        assert getattr(lib, n)(0, None, None, None, None, None, None) == 1      # wrong parameter count, before anything else


def test_ctypes_mirrors_have_the_headers_layout():
    task = type("Task", (C.Structure,), {"_fields_": _struct_fields("md_cp_task_attrs", {})})
    head = type("Head", (C.Structure,), {"_fields_": _struct_fields("md_cp_head_attrs", {"md_cp_task_attrs": task})})
    nms = type("Nms", (C.Structure,), {"_fields_": _struct_fields("md_nms_rotated_attrs", {})})
    assert C.sizeof(task) == 32 and C.sizeof(head) == 4 + 8 * 32 + 12 * 4 + 4 and C.sizeof(nms) == 12

    def layout(s):
        return [(n, getattr(s, n).offset, getattr(s, n).size) for n, _ in s._fields_]

    for want, mirrors in ((head, (det_ops._CPHeadAttrs, CPHead)), (nms, (det_ops._NmsRotatedAttrs, NmsRotated)),
                          (task, (det_ops._CPTaskAttrs,))):
        for got in mirrors:
            assert C.sizeof(got) == C.sizeof(want) and layout(got) == layout(want), got
    assert dict(det_ops._CPHeadAttrs._fields_)["task"]._type_ is det_ops._CPTaskAttrs and det_ops.CP_MAX_TASKS == 8


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    lib = _lib_handle()
    muts = mutations(case)
    kinds = {k for k, _, _, _ in muts}
    assert {"nparam", "params_null", "ndims_null", "shapes_null", "extra_null", "shape_null", "ptr_null", "dtype", "rank-1", "rank+1"} <= kinds
    bad = [(kind, i, rc, want) for kind, i, call, want in muts for rc in [call.run(lib)] if rc != want]
    assert not bad, f"{case.id}: (defect, operand, rc, expected) {bad}"


def _rc(case, edit):
    c = copy.copy(case)
    c.extra = type(case.extra).from_buffer_copy(case.extra)
    c.operands = list(case.operands)
    edit(c)
    return Call(c).run(_lib_handle())


def test_semantic_refusals_return_the_documented_codes():
    by = {c.id: c for c in CASES}
    ARG, SIZE = 2, 4

    def attr(name, value):
        return lambda c: setattr(c.extra, name, value)

    def task(t, name, value):
        return lambda c: setattr(c.extra.task[t], name, value)

    def shape(i, shp, dtype=F):
        def edit(c):
            c.operands[i] = T(shp, dtype)
        return edit

    nms = by["md_nms_rotated[count]"]
    for e in (attr("mode", 2), attr("mode", -1), attr("max_output", -1), shape(0, (2, 4, 6)), shape(1, (3,), I), shape(2, (2, 5), I),
              shape(3, (3,), I)):
        assert _rc(nms, e) == ARG
    for e in (shape(0, (2, 65537, 7)), shape(0, (65536, 1, 7))):
        assert _rc(nms, e) == SIZE
    sc, dec, pack = by["md_cp_scores"], by["md_cp_decode_selected"], by["md_cp_pack"]
    head_edits = (attr("num_tasks", 0), attr("num_tasks", 9), task(0, "num_classes", 0), task(1, "off_hm", 23), task(1, "off_hm", -1),
                  task(0, "off_vel", -2), task(0, "off_vel", 23), task(1, "off_dim", 22), task(0, "off_reg", -1), task(1, "off_rot", 23),
                  task(0, "off_height", 24))
    for e in head_edits + (shape(1, (1, 3, 16)), shape(1, (1, 2, 15)), shape(1, (2, 2, 16))):
        assert _rc(sc, e) == ARG
    assert _rc(sc, shape(0, (1, 4, 4, 488), "bfloat16")) == SIZE
    for e in head_edits + (shape(1, (1, 3, 3), I), shape(1, (2, 2, 3), I), shape(2, (1, 3), I), shape(3, (1, 2, 3, 8)), shape(3, (1, 2, 4, 9)),
                           shape(4, (1, 2, 3, 9)), shape(5, (1, 2, 4), I)):
        assert _rc(dec, e) == ARG
    for e in (attr("num_tasks", 3), attr("num_tasks", 0), attr("max_per_task", -1), attr("max_per_task", 3), shape(0, (1, 2, 3, 8)),
              shape(1, (1, 2, 4)), shape(2, (1, 3, 3), I), shape(3, (2, 2, 3), I), shape(4, (1, 3), I), shape(5, (2, 2), I), shape(6, (1, 4, 10)),
              shape(6, (1, 5, 11)), shape(7, (2,), I)):
        assert _rc(pack, e) == ARG


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
