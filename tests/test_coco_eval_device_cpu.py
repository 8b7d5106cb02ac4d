"""CPU: the COCO bbox AP operators without a GPU -- the ABI of include/minddet_hip_cocoeval.h (the three functions exported, header and
Makefile wired, every documented rc 2 / rc 4 and aliasing answered before any device call, the ctypes mirrors
and limits laid out as the header says), the Python layer's refusals, coco_eval.pack_coco against what COCOBboxEval groups, the contract
(tests/coco_eval_contract.py) against COCOBboxEval.evaluate() bit for bit, the to_float recipe against Python's formatting, and the six
planted defects, each of which must change the contract's tables on the test set."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from minddet_amd import _lib, det_ops
from minddet_amd import coco_eval as ce
from tests import coco_eval_contract as cc
from tests import abi_header as ah
from tests.abi_cases_cocoeval import CASES, CELLS, DT, GT, KC, MAX_DET, NA, NI, NM, NR, NT, RowsAttrs
from tests.abi_derive import attr, edited, lib_handle, rc, refuse_single_defects, shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["md_coco_eval_rows", "md_coco_eval_match", "md_coco_eval_accumulate"]
ARG, SIZE = 2, 4
BY_ID = {c.id: c for c in CASES}
EV = ce.COCOBboxEval
AREA = np.array(list(EV.AREA_RNG.values()), np.float64)


def test_header_declares_the_symbols_and_the_library_exports_them():
    hdr = ah.header("minddet_hip_cocoeval.h")
    assert ah.aot_symbols(hdr) == SYMS and "_workspace_bytes" not in hdr
    for cite in ("post_process.py:64-89", "centernet/eval.py:181-187", "fma(v, 100, -p)", "the highest row on equal IoU"):
        assert cite in hdr, cite
    mk = open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    assert "minddet_hip_cocoeval.h" in mk
    src = open(os.path.join(ROOT, "minddet_amd", "csrc", "cocoeval.hip")).read()
    assert src.index("#pragma clang fp contract(off)") < src.index('#include "aot.h"') and ".acquire(" not in src and not re.search(r"atomic\w*\(", src)
    assert '#include "workgroup.h"' in src and "hipMemset" not in src
    assert {c.sym for c in CASES} == set(SYMS) and len({c.id for c in CASES}) == len(CASES)
    lib = lib_handle()
    for sym in SYMS:
        assert getattr(lib, sym)(0, None, None, None, None, None, None) == 1      # wrong parameter count, before anything else
        assert sym not in _lib.exported_symbols()                                  # declared in the new header only
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "minddet_hip_cocoeval.h":
            assert "md_coco_eval" not in open(os.path.join(ROOT, "include", other)).read(), other


def test_ctypes_mirrors_and_limits_have_the_headers_layout():
    hdr = ah.header("minddet_hip_cocoeval.h")
    assert ah.statements("md_coco_eval_rows_attrs", hdr) == ["int32_t first_image"]
    for got in (det_ops._CocoEvalRowsAttrs, RowsAttrs):
        assert C.sizeof(got) == 4 and got.first_image.offset == 0
    macros = {k[len("MD_COCOEVAL_"):]: v for k, v in ah.defines(hdr).items() if k.startswith("MD_COCOEVAL_")}
    assert set(macros) == {"MAX_DETS", "MAX_GTS", "MAX_IMAGE_DETS", "MAX_CELLS", "MAX_CATS", "MAX_ROWS", "MAX_LABELS", "MAX_THRS", "MAX_AREAS", "MAX_RECS",
                           "MAX_MAXDETS"}
    for name, v in macros.items():
        assert getattr(det_ops, "COCOEVAL_" + name) == v, name
    assert (ce.MAX_CELL_DETS, ce.MAX_CELL_GTS, ce.MAX_IMAGE_DETS) == (macros["MAX_DETS"], macros["MAX_GTS"], macros["MAX_IMAGE_DETS"]) == (100, 256, 512)
    assert macros["MAX_CELLS"] == 1 << 24 and macros["MAX_CATS"] == 128 and EV.MAX_DETS[-1] == macros["MAX_DETS"] == cc.MAX_CELL_DETS
    assert (len(EV.IOU_THRS), len(EV.REC_THRS), len(EV.AREA_RNG), len(EV.MAX_DETS)) == (NT, NR, NA, NM)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_cocoeval", case)


def _described(case, shapes):
    """the call of `case` with the shapes of some operands replaced in the description alone (the host blocks stay small: a refused
    call touches nothing)"""
    call = edited(case, lambda c: None)
    for i, shp in shapes.items():
        call.shapes[i] = list(shp)
    return call.run(lib_handle())


def test_semantic_refusals_return_the_documented_codes():
    rows, match, accum = BY_ID["md_coco_eval_rows[whole set]"], BY_ID["md_coco_eval_match"], BY_ID["md_coco_eval_accumulate"]
    # every extent that disagrees: rc 2
    for i, e in enumerate([shape(0, (NI, MAX_DET, 5)), shape(0, (NI, 3, 6)), shape(1, (NI + 1,)), shape(3, (DT, 3)), shape(3, (DT + 1, 4)), shape(4, (DT - 1,)),
                           shape(5, (DT + 1,)), shape(6, (DT - 1,)), shape(7, (DT + 1,)), shape(8, (CELLS + 1,)), shape(9, (CELLS - 1,)), shape(10, (DT + 1,)),
                           shape(0, (NI + 1, MAX_DET, 6)), attr("first_image", -1), attr("first_image", 1), attr("first_image", NI)]):
        assert rc(rows, e) == ARG, i
    assert _described(rows, {8: (CELLS + 1,), 9: (CELLS + 1,)}) == ARG             # seven cells over two images
    for i, e in enumerate([shape(1, (CELLS + 1,)), shape(2, (CELLS - 1,)), shape(3, (CELLS + 1,)), shape(4, (GT, 5)), shape(5, (GT + 1,)), shape(6, (GT - 1,)),
                           shape(7, (GT + 1,)), shape(8, (DT, 5)), shape(9, (DT + 1,)), shape(11, (NA, 3)), shape(11, (NA + 1, 2)), shape(10, (NT + 1,)),
                           shape(12, (NA, NT, DT + 1)), shape(13, (NA, NT + 1, DT)), shape(13, (NA + 1, NT, DT)), shape(14, (NA, CELLS + 1)),
                           shape(14, (NA + 1, CELLS))]):
        assert rc(match, e) == ARG, i
    for i, e in enumerate([shape(0, (DT + 1,)), shape(2, (DT - 1,)), shape(1, (KC + 2,)), shape(1, (1,)), shape(4, (NA, NT, DT + 1)), shape(4, (NA, NT + 1, DT)),
                           shape(5, (NA + 1, CELLS)), shape(5, (NA, CELLS + 1)), shape(6, (NR + 1,)), shape(7, (NM + 1,)), shape(8, (NT, NR, KC, NA, NM + 1)),
                           shape(8, (NT, NR, KC + 1, NA, NM)), shape(9, (NT, KC, NA + 1, NM)), shape(9, (NT + 1, KC, NA, NM)), shape(10, (NA, KC + 1)),
                           shape(10, (NA + 1, KC))]):
        assert rc(accum, e) == ARG, i
    # every documented limit: rc 4 (the descriptions alone say so)
    D = det_ops
    md1 = D.COCOEVAL_MAX_IMAGE_DETS + 1
    assert _described(rows, {0: (NI, md1, 6), **{i: (NI * md1,) for i in (4, 5, 6, 7, 10)}, 3: (NI * md1, 4)}) == SIZE
    assert _described(rows, {2: (D.COCOEVAL_MAX_LABELS + 1,)}) == SIZE
    k1 = D.COCOEVAL_MAX_CATS + 1
    assert _described(rows, {8: (NI * k1,), 9: (NI * k1,)}) == SIZE
    i1 = D.COCOEVAL_MAX_CELLS // KC + 1                                            # images: 3 i1 cells are 2^24 or more
    assert i1 * MAX_DET <= D.COCOEVAL_MAX_ROWS and i1 * KC >= D.COCOEVAL_MAX_CELLS
    assert _described(rows, {8: (i1 * KC,), 9: (i1 * KC,), **{i: (i1 * MAX_DET,) for i in (4, 5, 6, 7, 10)}, 3: (i1 * MAX_DET, 4)}) == SIZE
    r1 = D.COCOEVAL_MAX_ROWS + MAX_DET
    assert _described(rows, {8: (r1 // MAX_DET * KC,), 9: (r1 // MAX_DET * KC,), **{i: (r1,) for i in (4, 5, 6, 7, 10)}, 3: (r1, 4)}) == SIZE
    c1 = D.COCOEVAL_MAX_CELLS
    assert _described(match, {0: (c1,), 1: (c1,), 2: (c1,), 3: (c1,), 14: (NA, c1)}) == SIZE
    g1 = D.COCOEVAL_MAX_ROWS + 1
    assert _described(match, {4: (g1, 4), 5: (g1,), 6: (g1,), 7: (g1,)}) == SIZE
    assert _described(match, {8: (g1, 4), 9: (g1,), 12: (NA, NT, g1), 13: (NA, NT, g1)}) == SIZE
    t1, a1 = D.COCOEVAL_MAX_THRS + 1, D.COCOEVAL_MAX_AREAS + 1
    assert _described(match, {10: (t1,), 12: (NA, t1, DT), 13: (NA, t1, DT)}) == SIZE
    assert _described(match, {11: (a1, 2), 12: (a1, NT, DT), 13: (a1, NT, DT), 14: (a1, CELLS)}) == SIZE
    big = (1 << 31) // (NA * NT) + 1                                               # A T Dt reaches 2^31 below the row limit
    assert big <= D.COCOEVAL_MAX_ROWS
    assert _described(match, {8: (big, 4), 9: (big,), 12: (NA, NT, big), 13: (NA, NT, big)}) == SIZE
    assert _described(accum, {1: (k1 + 1,), 5: (NA, k1 * NI), 8: (NT, NR, k1, NA, NM), 9: (NT, k1, NA, NM), 10: (NA, k1)}) == SIZE
    assert _described(accum, {5: (NA, c1 // KC * KC + KC)}) == SIZE
    assert _described(accum, {0: (g1,), 2: (g1,), 3: (NA, NT, g1), 4: (NA, NT, g1)}) == SIZE
    assert _described(accum, {6: (D.COCOEVAL_MAX_RECS + 1,), 8: (NT, D.COCOEVAL_MAX_RECS + 1, KC, NA, NM)}) == SIZE
    m1 = D.COCOEVAL_MAX_MAXDETS + 1
    assert _described(accum, {7: (m1,), 8: (NT, NR, KC, NA, m1), 9: (NT, KC, NA, m1)}) == SIZE
    assert _described(accum, {3: (NA, t1, DT), 4: (NA, t1, DT), 8: (t1, NR, KC, NA, NM), 9: (t1, KC, NA, NM)}) == SIZE
    assert _described(accum, {5: (NA, CELLS + 1)}) == ARG                          # seven cells over three categories


def test_aliased_outputs_are_refused():
    """an output at the address of an input or of another output: rc 2 before any device call"""
    lib = lib_handle()
    for cid, pairs in (("md_coco_eval_rows[whole set]", ((3, 0), (6, 1), (7, 6), (9, 8), (10, 2), (5, 4))),
                       ("md_coco_eval_match", ((12, 0), (13, 6), (13, 12), (14, 3), (14, 12))),
                       ("md_coco_eval_accumulate", ((8, 6), (9, 8), (10, 5), (10, 1)))):
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


def test_python_layer_refuses_before_any_device_call():
    gts, dts, imgs, cats, _ = cc.test_set()
    crowded = [dict(image_id=1, category_id=1, bbox=[0.0, 0.0, 4.0, 4.0])] * (ce.MAX_CELL_GTS + 1)
    with pytest.raises(ValueError):
        ce.pack_coco(crowded, [], device="cpu")                                   # a cell beyond 256 ground truths
    ce.pack_coco(crowded[:-1], [], device="cpu")
    with pytest.raises(ValueError):
        ce.pack_coco(gts, dts, imgs, list(range(1, 131)), device="cpu")           # more than 128 categories
    p = ce.pack_coco(gts, None, imgs, cats, device="cpu")
    assert p.dt_box is None and p.gt_box.shape[1] == 4
    for bad in (torch.zeros((2, ce.MAX_IMAGE_DETS + 1, 6)), torch.zeros((2, 8, 5)), torch.zeros((8, 6))):
        with pytest.raises(ValueError):
            p.add_dets(bad, torch.zeros((2,), dtype=torch.int32), 0)
    with pytest.raises(ValueError):
        p.add_dets(torch.zeros((2, 8, 6)), torch.zeros((2,), dtype=torch.int32), len(imgs) - 1)      # the batch leaves the image list
    with pytest.raises(ValueError):
        p.add_dets(torch.zeros((2, 8, 6)), torch.zeros((2,), dtype=torch.int32), -1)
    with pytest.raises(ValueError):
        EV.from_packed(p).evaluate(backend="device")                              # no detections yet
    with pytest.raises(ValueError):
        EV.from_packed(p).evaluate()                                              # no host records
    with pytest.raises(ValueError):
        EV(gts, dts, imgs, cats).evaluate(backend="numpy")
    with pytest.raises(ValueError):
        ce.pack_coco(gts, dts, imgs, cats, device="cpu").add_dets(torch.zeros((2, 8, 6)), torch.zeros((2,), dtype=torch.int32), 0)
    # the thin wrappers check shapes and limits first
    f64, u8, i32t = torch.float64, torch.uint8, torch.int32
    z = lambda *s, dtype=f64: torch.zeros(s, dtype=dtype)
    outs = lambda Dt=8, Cn=6: [z(Dt, 4), z(Dt), z(Dt), z(Dt, dtype=i32t), z(Dt, dtype=i32t), z(Cn, dtype=i32t), z(Cn, dtype=i32t), z(Dt, dtype=i32t)]
    f32 = torch.float32
    for args in ([z(2, 4, 5, dtype=f32), z(2, dtype=i32t), z(3, dtype=i32t), 0] + outs(), [z(2, 4, 6), z(2, dtype=i32t), z(3, dtype=i32t), 0] + outs(),
                 [z(2, 4, 6, dtype=f32), z(3, dtype=i32t), z(3, dtype=i32t), 0] + outs(), [z(2, 4, 6, dtype=f32), z(2, dtype=i32t), z(3, dtype=i32t), 1] + outs(),
                 [z(2, 4, 6, dtype=f32), z(2, dtype=i32t), z(3, dtype=i32t), 0] + outs(Dt=9), [z(2, 4, 6, dtype=f32), z(2, dtype=i32t), z(3, dtype=i32t), 0] + outs(Cn=7),
                 [z(2, 513, 6, dtype=f32), z(2, dtype=i32t), z(3, dtype=i32t), 0] + outs(Dt=1026), [z(2, 4, 6, dtype=f32), z(2, dtype=i32t), z(0, dtype=i32t), 0] + outs(),
                 [z(2, 4, 6, dtype=f32), z(2, dtype=i32t), z(3, dtype=i32t), 0] + outs()[:3] + [z(8)] + outs()[4:],
                 [z(2, 4, 6, dtype=f32), z(2, dtype=i32t), z(3, dtype=i32t), 0] + outs(Cn=2 * 129)):
        with pytest.raises(ValueError):
            det_ops.coco_eval_rows(*args)
    cells = [z(6, dtype=i32t)] * 4
    m = cells + [z(5, 4), z(5), z(5, dtype=u8), z(5, dtype=u8), z(8, 4), z(8), z(10), z(4, 2)]
    for i, bad in ((1, z(7, dtype=i32t)), (4, z(5, 5)), (5, z(6)), (7, z(4, dtype=u8)), (8, z(8, 3)), (9, z(7)), (10, z(17)), (11, z(4, 3)), (11, z(9, 2))):
        with pytest.raises(ValueError):
            det_ops.coco_eval_match(*[bad if j == i else t for j, t in enumerate(m)])
    acc = [z(8, dtype=i32t), z(4, dtype=i32t), z(8, dtype=i32t), z(4, 10, 8, dtype=i32t), z(4, 10, 8, dtype=u8), z(4, 6, dtype=i32t), z(101), z(3, dtype=i32t)]
    for i, bad in ((0, z(9, dtype=i32t)), (1, z(1, dtype=i32t)), (1, z(5, dtype=i32t)), (2, z(7, dtype=i32t)), (4, z(4, 9, 8, dtype=u8)), (5, z(3, 6, dtype=i32t)),
                   (6, z(257)), (7, z(9, dtype=i32t))):
        with pytest.raises(ValueError):
            det_ops.coco_eval_accumulate(*[bad if j == i else t for j, t in enumerate(acc)])


@functools.lru_cache(maxsize=None)
def _host():
    """the test set, its host evaluator after evaluate(), its pack on the CPU as numpy arrays"""
    gts, dts, imgs, cats, where = cc.test_set()
    ev = EV(gts, dts, imgs, cats).evaluate()
    return ev, cc.pack_numpy(ce.pack_coco(gts, dts, imgs, cats, device="cpu")), where


@functools.lru_cache(maxsize=None)
def _contract(defect=None):
    ev, z, _ = _host()
    return cc.tables(z, len(ev.cat_ids), EV.IOU_THRS, EV.REC_THRS, AREA, np.array(EV.MAX_DETS), defect)


def test_pack_coco_cells_order_and_ranks_equal_what_the_evaluator_groups():
    ev, z, where = _host()
    I, Kc = len(ev.img_ids), len(ev.cat_ids)
    assert z["gt_beg"].shape == z["dt_cnt"].shape == (I * Kc,) and z["gt_box"].dtype == z["dt_score"].dtype == np.float64
    assert z["gt_beg"].dtype == z["dt_cat"].dtype == z["dt_rank"].dtype == np.int32 and z["gt_crowd"].dtype == z["gt_ignore"].dtype == np.uint8
    g_at = d_at = 0
    for i, img in enumerate(ev.img_ids):
        for k, cat in enumerate(ev.cat_ids):
            c = i * Kc + k
            gts, dts = ev.gts.get((img, cat), []), ev.dts.get((img, cat), [])
            dts = [dts[j] for j in np.argsort([-d["score"] for d in dts], kind="mergesort")[:100]]
            assert (z["gt_beg"][c], z["gt_cnt"][c], z["dt_beg"][c], z["dt_cnt"][c]) == (g_at, len(gts), d_at, len(dts)), (img, cat)
            gs, ds = slice(g_at, g_at + len(gts)), slice(d_at, d_at + len(dts))
            assert np.array_equal(z["gt_box"][gs], np.array([g["bbox"] for g in gts], float).reshape(-1, 4))
            assert z["gt_area"][gs].tolist() == [g["area"] for g in gts] and z["gt_crowd"][gs].tolist() == [int(bool(g["iscrowd"])) for g in gts]
            assert z["gt_ignore"][gs].tolist() == [int(g["_ignore"]) for g in gts]
            assert np.array_equal(z["dt_box"][ds], np.array([d["bbox"] for d in dts], float).reshape(-1, 4))
            assert z["dt_score"][ds].tolist() == [d["score"] for d in dts] and z["dt_area"][ds].tolist() == [d["area"] for d in dts]
            assert z["dt_cat"][ds].tolist() == [k] * len(dts) and z["dt_rank"][ds].tolist() == list(range(len(dts)))
            g_at, d_at = g_at + len(gts), d_at + len(dts)
    assert g_at == len(z["gt_area"]) and d_at == len(z["dt_area"])
    cell = lambda name: ev.img_ids.index(where[name][0]) * Kc + ev.cat_ids.index(where[name][1])
    assert z["dt_cnt"][cell("dets_140")] == 100 and z["gt_cnt"][cell("gts_256")] == 256 and z["gt_cnt"][cell("dets_only")] == 0
    assert z["gt_cnt"][ev.img_ids.index(99) * Kc:(ev.img_ids.index(99) + 1) * Kc].sum() == 0 and (z["gt_ignore"] > z["gt_crowd"]).any()
    # the order operand: category-major, descending score, equal scores in row order
    p = ce.pack_coco(*cc.test_set()[:4], device="cpu")
    order, cat_off = (t.numpy() for t in p.category_order())
    want = sorted(range(len(z["dt_cat"])), key=lambda r: (z["dt_cat"][r], -z["dt_score"][r], r))
    assert order.tolist() == want and cat_off.tolist() == [0] + np.cumsum(np.bincount(z["dt_cat"], minlength=Kc)).tolist()


def test_contract_tables_equal_the_host_evaluator_bit_for_bit():
    ev, z, _ = _host()
    got = _contract()
    assert got["precision"].shape == ev.precision.shape and np.array_equal(got["precision"].view(np.int64), ev.precision.view(np.int64))
    assert np.array_equal(got["recall"].view(np.int64), ev.recall.view(np.int64))
    assert 0.1 < ev.summarize()["AP"] < 0.9 and (ev.precision[:, :, 3] == -1).all() and (ev.precision[:, :, 4, 0] == 0).all()      # not a trivial set
    # the match tables against _evaluate_img, the host's index mapped back through its ground-truth order
    Kc = len(ev.cat_ids)
    for i, img in enumerate(ev.img_ids):
        for k, cat in enumerate(ev.cat_ids):
            c = i * Kc + k
            for a, rng in enumerate(EV.AREA_RNG.values()):
                e = ev._evaluate_img(img, cat, rng, 100)
                ds = slice(z["dt_beg"][c], z["dt_beg"][c] + z["dt_cnt"][c])
                if e is None:
                    assert z["gt_cnt"][c] == 0 and z["dt_cnt"][c] == 0
                    continue
                gts = ev.gts.get((img, cat), [])
                g_ig = np.array([g["_ignore"] or g["area"] < rng[0] or g["area"] > rng[1] for g in gts], bool)
                back = np.append(np.argsort(g_ig, kind="mergesort") + z["gt_beg"][c], -1)
                assert np.array_equal(got["dtm"][a][:, ds], back[e["dtm"]]), (img, cat, a)
                assert np.array_equal(got["dt_ig"][a][:, ds] != 0, e["dt_ig"]) and got["cell_ngt"][a, c] == e["n_gt"]


def test_to_float_recipe_equals_pythons_formatting():
    rng = np.random.default_rng(3)
    coords = (rng.uniform(-50, 1400, 6000)).astype(np.float32)
    vals = [float(v) for v in coords] + [float(np.float64(a) - np.float64(b)) for a, b in zip(coords[:3000], coords[3000:])]
    vals += [k / 8 for k in range(-4000, 4001)] + [k / 8 + 1000 for k in range(0, 800)] + [0.0, -0.0, 0.005, -0.005, 0.015, 0.025, 1e-9, -1e-9, 2.675, 1.005]
    vals += [float(np.float32(s)) for s in rng.uniform(0, 1, 4000)] + [float(np.float32(k / 200)) for k in range(0, 201)]
    for v in vals:
        want, got = ce.to_float(v), cc.to_float_recipe(v)
        assert got == want and np.signbit(got) == np.signbit(want), (v, got, want)
    assert ce.to_float(0.125) == 0.12 and ce.to_float(0.375) == 0.38 and str(cc.to_float_recipe(-0.001)) == "-0.0"


def test_rows_contract_equals_dets_to_coco_and_pack_coco():
    """rows_image against the host path it restates, on f32 detections with k/8 coordinates, tied scores, a dropped label and a full cell"""
    rng = np.random.default_rng(5)
    dets = np.zeros((3, 160, 6), np.float32)
    dets[..., :2] = rng.integers(0, 800, (3, 160, 2)) / 8
    dets[..., 2:4] = dets[..., :2] + rng.integers(1, 900, (3, 160, 2)) / 8
    dets[..., 4] = rng.choice([0.125, 0.375, 0.625, 0.3, 0.9, 0.905], (3, 160))
    dets[..., 5] = rng.integers(0, 4, (3, 160))
    dets[1, :130, 5] = 3                                                         # more than 100 rows of one class
    count, valid_ids, cat_ids = [160, 150, 0], [10, 20, 77, 40], [10, 20, 40]    # label 2 has no category: dropped
    ref = ce.dets_to_coco(dets, count, [5, 6, 7], valid_ids)
    z = cc.pack_numpy(ce.pack_coco([], [r for r in ref if r["category_id"] in cat_ids], [5, 6, 7], cat_ids, device="cpu"))
    at = 0
    for b in range(3):
        got = cc.rows_image(dets[b], count[b], [0, 1, -1, 2], 3)
        n = int(got["cnt"].sum())
        assert got["cnt"].tolist() == z["dt_cnt"][b * 3:b * 3 + 3].tolist() and (got["beg"] + at).tolist() == z["dt_beg"][b * 3:b * 3 + 3].tolist()
        for name, key in (("box", "dt_box"), ("area", "dt_area"), ("score", "dt_score"), ("cat", "dt_cat"), ("rank", "dt_rank")):
            assert np.array_equal(got[name][:n], z[key][at:at + n]), (b, name)
        assert (got["cat"][n:] == 3).all() and (got["src"][n:] == -1).all() and len(set(got["src"][:n].tolist())) == n
        at += n
    assert at == len(z["dt_area"]) and z["dt_cnt"][5] == 100 and z["dt_cnt"][6:].sum() == 0


@pytest.mark.parametrize("defect", cc.DEFECTS)
def test_each_planted_defect_changes_the_tables(defect):
    good, bad = _contract(), _contract(defect)
    changed = [n for n in ("dtm", "dt_ig", "cell_ngt", "precision", "recall") if not np.array_equal(good[n], bad[n])]
    assert changed, f"the test set does not see {defect}: strengthen it"
    assert "precision" in changed or "recall" in changed or defect == "lowest_row", (defect, changed)
