"""CPU: the nuScenes evaluation operators without a GPU -- the ABI of include/minddet_hip_nusceval.h (the three functions exported, header
and Makefile wired, every documented rc 2 / rc 4 and aliasing answered before any device call, the ctypes mirrors
and limits laid out as the header says), the Python layer's refusals, the contract (tests/nusc_eval_contract.py) against
NuscDetectionEval.evaluate() bit for bit on the test set, the rows contract against dets_to_nusc and pack_nusc, the element rule of
interp against np.interp, the eight planted defects, each of which must change the contract's tables, and summarize() on a hand-computed
two-class case."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from minddet_amd import det_ops
from minddet_amd import nusc_eval as ne
from tests import nusc_eval_contract as nc
from tests import abi_header as ah
from tests.abi_cases_nusceval import CASES, CELLS, DT, GT, KC, MAX_DET, ND, NI, NR, EvalAttrs, RowsAttrs
from tests.abi_derive import attr, edited, lib_handle, rc, refuse_single_defects, shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["md_nusc_rows", "md_nusc_eval_match", "md_nusc_eval_accumulate"]
ARG, SIZE = 2, 4
BY_ID = {c.id: c for c in CASES}
REC = np.linspace(0, 1, 101)


def test_header_declares_the_symbols_and_the_library_exports_them():
    hdr = ah.header("minddet_hip_nusceval.h")
    assert ah.aot_symbols(hdr) == SYMS and "_workspace_bytes" not in hdr
    for cite in ("nusc_common.py:160-201", "nuscenes.py:252-293", "nusc_common.py:659-674", "the lowest row on equal distance", "np.cumsum's bits"):
        assert cite in hdr, cite
    mk = open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    assert "minddet_hip_nusceval.h" in mk
    src = open(os.path.join(ROOT, "minddet_amd", "csrc", "nusceval.hip")).read()
    assert src.index("#pragma clang fp contract(off)") < src.index('#include "aot.h"') and ".acquire(" not in src and not re.search(r"atomic\w*\(", src)
    assert '#include "workgroup.h"' in src and "hipMemset" not in src
    assert {c.sym for c in CASES} == set(SYMS) and len({c.id for c in CASES}) == len(CASES)
    lib = lib_handle()
    for sym in SYMS:
        assert getattr(lib, sym)(0, None, None, None, None, None, None) == 1      # wrong parameter count, before anything else
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "minddet_hip_nusceval.h":
            assert "md_nusc_" not in open(os.path.join(ROOT, "include", other)).read(), other


def test_ctypes_mirrors_and_limits_have_the_headers_layout():
    hdr = ah.header("minddet_hip_nusceval.h")
    for struct, field, mirrors in (("md_nusc_rows_attrs", "first_sample", (det_ops._NuscRowsAttrs, RowsAttrs)),
                                   ("md_nusc_eval_attrs", "tp_index", (det_ops._NuscEvalAttrs, EvalAttrs))):
        assert ah.statements(struct, hdr) == ["int32_t " + field]
        for got in mirrors:
            assert C.sizeof(got) == 4 and getattr(got, field).offset == 0
    macros = {k[len("MD_NUSCEVAL_"):]: v for k, v in ah.defines(hdr).items() if k.startswith("MD_NUSCEVAL_")}
    assert set(macros) == {"MAX_SAMPLE_DETS", "MAX_GTS", "MAX_CLASSES", "MAX_THRS", "MAX_RECS", "MAX_CELLS", "MAX_ROWS", "MAX_LABELS"}
    for name, v in macros.items():
        assert getattr(det_ops, "NUSCEVAL_" + name) == v, name
    assert (ne.MAX_SAMPLE_DETS, ne.MAX_CELL_GTS, ne.MAX_CLASSES, ne.MAX_THRS) == (macros["MAX_SAMPLE_DETS"], macros["MAX_GTS"], macros["MAX_CLASSES"],
                                                                                  macros["MAX_THRS"]) == (512, 1024, 16, 8)
    cfg = ne.DETECTION_CVPR_2019
    assert cfg["max_boxes_per_sample"] == 500 <= macros["MAX_SAMPLE_DETS"] and len(cfg["dist_ths"]) == ND and len(cfg["class_range"]) == 10
    assert cfg["dist_ths"].index(cfg["dist_th_tp"]) == 2 and len(ne.ATTRIBUTES) == 8 and set(ne.DEFAULT_ATTR) == set(cfg["class_range"])


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_nusceval", case)


def _described(case, shapes):
    """the call of `case` with the shapes of some operands replaced in the description alone (the host blocks stay small: a refused
    call touches nothing)"""
    call = edited(case, lambda c: None)
    for i, shp in shapes.items():
        call.shapes[i] = list(shp)
    return call.run(lib_handle())


def test_semantic_refusals_return_the_documented_codes():
    rows, match, accum = BY_ID["md_nusc_rows[whole set]"], BY_ID["md_nusc_eval_match"], BY_ID["md_nusc_eval_accumulate"]
    # every extent that disagrees: rc 2
    for i, e in enumerate([shape(0, (NI, MAX_DET, 10)), shape(0, (NI, 3, 11)), shape(1, (NI + 1,)), shape(2, (NI, 13)), shape(2, (NI + 1, 14)),
                           shape(5, (KC + 1,)), shape(6, (KC - 1,)), shape(7, (DT, 4)), shape(8, (DT + 1, 3)), shape(9, (DT, 3)), shape(10, (DT, 3)),
                           shape(11, (DT + 1,)), shape(12, (DT - 1,)), shape(13, (DT + 1,)), shape(14, (DT - 1,)), shape(15, (DT + 1,)),
                           shape(16, (DT - 1,)), shape(17, (CELLS + 1,)), shape(18, (CELLS - 1,)), shape(0, (NI + 1, MAX_DET, 11)),
                           attr("first_sample", -1), attr("first_sample", 1), attr("first_sample", NI)]):
        assert rc(rows, e) == ARG, i
    assert _described(rows, {17: (CELLS + 3,), 18: (CELLS + 3,)}) == ARG            # nine cells over two samples of three classes
    for i, e in enumerate([shape(1, (CELLS + 1,)), shape(2, (CELLS - 1,)), shape(3, (CELLS + 1,)), shape(4, (GT, 3)), shape(5, (GT, 2)), shape(5, (GT + 1, 3)),
                           shape(6, (GT - 1,)), shape(7, (GT, 3)), shape(8, (GT + 1,)), shape(9, (DT, 2)), shape(10, (DT + 1, 3)), shape(11, (DT - 1,)),
                           shape(12, (DT, 3)), shape(13, (DT + 1,)), shape(16, (ND, DT + 1)), shape(16, (ND + 1, DT)), shape(17, (DT, 4)),
                           shape(17, (DT + 1, 5)), shape(18, (CELLS + 1,)), shape(15, (KC + 1,)), attr("tp_index", -1), attr("tp_index", ND)]):
        assert rc(match, e) == ARG, i
    for i, e in enumerate([shape(0, (DT + 1,)), shape(2, (DT - 1,)), shape(1, (KC + 2,)), shape(1, (1,)), shape(3, (ND, DT + 1)), shape(4, (DT, 4)),
                           shape(4, (DT + 1, 5)), shape(5, (CELLS + 1,)), shape(7, (KC, ND, NR + 1)), shape(8, (KC, ND + 1, NR)), shape(8, (KC + 1, ND, NR)),
                           shape(9, (KC, 4, NR)), shape(10, (KC + 1,)), shape(11, (KC, ND + 1)), shape(12, (ND, DT + 1)), shape(12, (ND + 1, DT)),
                           shape(13, (DT + 1,)), shape(14, (4, DT)), shape(14, (5, DT + 1)), attr("tp_index", -1), attr("tp_index", ND)]):
        assert rc(accum, e) == ARG, i
    # every documented limit: rc 4 (the descriptions alone say so)
    D = det_ops
    md1 = D.NUSCEVAL_MAX_SAMPLE_DETS + 1
    per_row = {7: 3, 8: 3, 9: 4, 10: 2}
    rows_dt = lambda n: {**{i: (n, w) for i, w in per_row.items()}, **{i: (n,) for i in range(11, 17)}}
    assert _described(rows, {0: (NI, md1, 11), **rows_dt(NI * md1)}) == SIZE
    assert _described(rows, {3: (D.NUSCEVAL_MAX_LABELS + 1,)}) == SIZE
    k1 = D.NUSCEVAL_MAX_CLASSES + 1
    assert _described(rows, {4: (k1,), 5: (k1,), 6: (k1,), 17: (NI * k1,), 18: (NI * k1,)}) == SIZE
    i1 = D.NUSCEVAL_MAX_CELLS // KC + 1                                            # samples: 3 i1 cells are 2^24 or more
    assert i1 * MAX_DET <= D.NUSCEVAL_MAX_ROWS and i1 * KC >= D.NUSCEVAL_MAX_CELLS
    assert _described(rows, {17: (i1 * KC,), 18: (i1 * KC,), **rows_dt(i1 * MAX_DET)}) == SIZE
    r1 = D.NUSCEVAL_MAX_ROWS + MAX_DET
    assert _described(rows, {17: (r1 // MAX_DET * KC,), 18: (r1 // MAX_DET * KC,), **rows_dt(r1)}) == SIZE
    c1 = D.NUSCEVAL_MAX_CELLS // KC * KC + KC
    assert _described(match, {0: (c1,), 1: (c1,), 2: (c1,), 3: (c1,), 18: (c1,)}) == SIZE
    g1 = D.NUSCEVAL_MAX_ROWS + 1
    assert _described(match, {4: (g1, 2), 5: (g1, 3), 6: (g1,), 7: (g1, 2), 8: (g1,)}) == SIZE
    assert _described(match, {9: (g1, 3), 10: (g1, 3), 11: (g1,), 12: (g1, 2), 13: (g1,), 16: (ND, g1), 17: (g1, 5)}) == SIZE
    t1 = D.NUSCEVAL_MAX_THRS + 1
    assert _described(match, {14: (t1,), 16: (t1, DT)}) == SIZE
    assert _described(match, {15: (k1,), 0: (NI * k1,), 1: (NI * k1,), 2: (NI * k1,), 3: (NI * k1,), 18: (NI * k1,)}) == SIZE
    assert _described(accum, {1: (k1 + 1,), 5: (k1 * NI,), 7: (k1, ND, NR), 8: (k1, ND, NR), 9: (k1, 5, NR), 10: (k1,), 11: (k1, ND)}) == SIZE
    assert _described(accum, {5: (c1,)}) == SIZE
    assert _described(accum, {0: (g1,), 2: (g1,), 3: (ND, g1), 4: (g1, 5), 12: (ND, g1), 13: (g1,), 14: (5, g1)}) == SIZE
    rr = D.NUSCEVAL_MAX_RECS + 1
    assert _described(accum, {6: (rr,), 7: (KC, ND, rr), 8: (KC, ND, rr), 9: (KC, 5, rr)}) == SIZE
    assert _described(accum, {3: (t1, DT), 7: (KC, t1, NR), 8: (KC, t1, NR), 11: (KC, t1), 12: (t1, DT)}) == SIZE
    assert _described(accum, {5: (CELLS + 1,)}) == ARG                              # seven cells over three classes


def test_aliased_outputs_are_refused():
    """an output at the address of an input or of another output: rc 2 before any device call"""
    lib = lib_handle()
    for cid, pairs in (("md_nusc_rows[whole set]", ((7, 0), (13, 1), (8, 7), (18, 17), (16, 3), (12, 11), (9, 2))),
                       ("md_nusc_eval_match", ((16, 0), (17, 4), (17, 16), (18, 3), (18, 16))),
                       ("md_nusc_eval_accumulate", ((7, 6), (8, 7), (10, 5), (12, 3), (14, 13), (13, 2)))):
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
            assert getattr(lib, case.sym)(n, params, ndims, shapes, dtypes, None, C.byref(case.extra)) == 2, (cid, out, other)


def test_python_layer_refuses_before_any_device_call():
    s = nc.test_set()
    gt1 = dict(s["gt_records"][0], sample_token=0)
    with pytest.raises(ValueError):
        ne.pack_nusc([gt1] * (ne.MAX_CELL_GTS + 1), s["ego"], nc.CLASSES, device="cpu")       # a cell beyond 1 024 ground truths
    ne.pack_nusc([gt1] * ne.MAX_CELL_GTS, s["ego"], nc.CLASSES, device="cpu")
    with pytest.raises(ValueError):
        ne.pack_nusc([], s["ego"], ["car"] * 17, device="cpu")                                # more than 16 classes
    d1 = dict(s["dt_records"][0], sample_token=0)
    with pytest.raises(ValueError):
        ne.NuscDetectionEval([], [d1] * 501, s["ego"], nc.CLASSES)                            # more than 500 predictions in a sample
    ne.NuscDetectionEval([], [d1] * 500, s["ego"], nc.CLASSES)
    with pytest.raises(ValueError):
        ne.NuscDetectionEval([], [dict(d1, detection_score=float("nan"))], s["ego"], nc.CLASSES)
    p = ne.pack_nusc(s["gt_records"], s["ego"], nc.CLASSES, device="cpu")
    assert p.dt_score is None and p.gt_xy.shape[1] == 2
    i32 = torch.int32
    for bad in (torch.zeros((2, 501, 11)), torch.zeros((2, 8, 10)), torch.zeros((8, 11))):
        with pytest.raises(ValueError):
            p.add_dets(bad, torch.zeros((2,), dtype=i32), np.zeros((2, 14)), 0)
    with pytest.raises(ValueError):
        p.add_dets(torch.zeros((2, 8, 11)), torch.zeros((2,), dtype=i32), np.zeros((2, 14)), nc.I - 1)      # the batch leaves the sample list
    with pytest.raises(ValueError):
        p.add_dets(torch.zeros((2, 8, 11)), torch.zeros((2,), dtype=i32), np.zeros((2, 14)), -1)
    with pytest.raises(ValueError):
        ne.NuscDetectionEval.from_packed(p).evaluate(backend="device")                        # no detections yet
    with pytest.raises(ValueError):
        ne.NuscDetectionEval.from_packed(p).evaluate()                                        # no host records
    with pytest.raises(ValueError):
        ne.NuscDetectionEval(s["gt_records"], s["dt_records"], s["ego"], nc.CLASSES).evaluate(backend="numpy")
    with pytest.raises(ValueError):
        ne.pack_nusc(s["gt_records"], s["ego"], nc.CLASSES, device="cpu", dt_records=s["dt_records"]).add_dets(
            torch.zeros((2, 8, 11)), torch.zeros((2,), dtype=i32), np.zeros((2, 14)), 0)
    # the thin wrappers check shapes and limits first
    f64, f32 = torch.float64, torch.float32
    z = lambda *sh, dtype=f64: torch.zeros(sh, dtype=dtype)
    ins = lambda B=2, M=4, L=3, Kc=3: [z(B, M, 11, dtype=f32), z(B, dtype=i32), z(B, 14), z(L, dtype=i32), z(Kc), z(Kc, dtype=i32), z(Kc, dtype=i32), 0]
    outs = lambda Dt=8, Cn=6: [z(Dt, 3), z(Dt, 3), z(Dt, 4), z(Dt, 2), z(Dt), z(Dt)] + [z(Dt, dtype=i32) for _ in range(4)] + [z(Cn, dtype=i32), z(Cn, dtype=i32)]
    bad_ins = ins()
    bad_ins[0] = z(2, 4, 11)                                                                   # float64 rows
    for args in (ins(M=513) + outs(Dt=1026), bad_ins + outs(), ins(L=0) + outs(), ins()[:7] + [1] + outs(), ins() + outs(Dt=9), ins() + outs(Cn=7),
                 ins() + outs()[:2] + [z(8, 3)] + outs()[3:], ins() + outs()[:6] + [z(8)] + outs()[7:], ins(Kc=17) + outs(Cn=34),
                 ins()[:2] + [z(2, 13)] + ins()[3:] + outs()):
        with pytest.raises(ValueError):
            det_ops.nusc_rows(*args)
    cells = [z(6, dtype=i32)] * 4
    m = cells + [z(5, 2), z(5, 3), z(5), z(5, 2), z(5, dtype=i32), z(8, 3), z(8, 3), z(8), z(8, 2), z(8, dtype=i32), z(4), z(3), 2]
    for i, bad in ((1, z(7, dtype=i32)), (4, z(5, 3)), (5, z(6, 3)), (7, z(5, 3)), (9, z(8, 2)), (11, z(7)), (14, z(9)), (15, z(4)), (15, z(17)), (16, 4), (16, -1)):
        with pytest.raises(ValueError):
            det_ops.nusc_eval_match(*[bad if j == i else t for j, t in enumerate(m)])
    acc = [z(8, dtype=i32), z(4, dtype=i32), z(8), z(4, 8, dtype=i32), z(8, 5), z(6, dtype=i32), z(101), 2]
    for i, bad in ((0, z(9, dtype=i32)), (1, z(1, dtype=i32)), (1, z(5, dtype=i32)), (2, z(7)), (4, z(8, 4)), (5, z(7, dtype=i32)), (6, z(257)), (7, 4)):
        with pytest.raises(ValueError):
            det_ops.nusc_eval_accumulate(*[bad if j == i else t for j, t in enumerate(acc)])


@functools.lru_cache(maxsize=None)
def _host():
    """the test set's host evaluator after evaluate()"""
    s = nc.test_set()
    return ne.NuscDetectionEval(s["gt_records"], s["dt_records"], s["ego"], nc.CLASSES).evaluate()


@functools.lru_cache(maxsize=None)
def _contract(defect=None):
    ev = _host()
    return nc.tables(ev.z, nc.KC, ev.cfg["dist_ths"], ev.periods(), REC, ev.tp_index(), defect)


def test_the_test_set_holds_what_it_was_made_for():
    ev, s = _host(), nc.test_set()
    z, t = ev.z, ev.tables
    car = z["gt_cnt"][0::nc.KC].tolist()
    assert {0, 1, 63, 64, 65, 130} <= set(car) and int(s["count"].max()) == 500 == nc.MAX_DET and 300 in z["dt_cnt"].tolist()
    k = nc.CLASSES.index
    assert t["n_gt"][k("trailer")] == 0 and z["dt_cnt"][k("trailer")::nc.KC].sum() > 0                       # a class without ground truth
    assert t["n_gt"][k("construction_vehicle")] > 0 and (t["n_match"][k("construction_vehicle")] == 0).all()  # ground truths, no match
    assert (z["gt_attr"] < 0).any() and np.isnan(z["gt_vel"]).any()
    for name in ("barrier", "traffic_cone"):                                                                  # every attr_err NaN: the curve is all ones
        hit = t["dtm"][ev.tp_index()][z["dt_cat"] == k(name)]
        assert (hit >= 0).any() and np.isnan(t["err"][z["dt_cat"] == k(name)][hit >= 0][:, 4]).all() and (t["tp_err"][k(name), 4] == 1).all()
    bar = t["err"][(z["dt_cat"] == k("barrier")) & (t["dtm"][ev.tp_index()] >= 0), 2]
    assert len(bar) and (bar <= np.pi / 2).all() and (bar > 1.0).any()                                        # turned by 2 rad: pi - 2 under the period pi
    # the hand-made pairs of sample 5: a distance exactly at a threshold misses it, the first of two equidistant ground truths wins
    rows5 = np.nonzero((z["dt_sample"] == 5) & (z["dt_cat"] == k("bicycle")))[0]
    d5 = {}
    for r in rows5:
        g0 = z["gt_beg"][5 * nc.KC + k("bicycle")]
        gs = z["gt_xy"][g0:g0 + z["gt_cnt"][5 * nc.KC + k("bicycle")]]
        d5[r] = np.sqrt(((z["dt_xyz"][r, :2] - gs) ** 2).sum(1)).min()
    assert {0.5, 1.0, 2.0, 4.0} <= set(d5.values())
    for r, dist in d5.items():
        if dist in (0.5, 1.0, 2.0, 4.0):
            assert [bool(t["dtm"][d, r] >= 0) for d in range(4)] == [dist < th for th in ev.cfg["dist_ths"]], (r, dist)
    mot = np.nonzero((z["dt_sample"] == 5) & (z["dt_cat"] == k("motorcycle")) & (z["dt_xyz"][:, 0] == s["poses"][5, 11] + 11.0))[0]
    g = int(t["dtm"][0, mot[0]])
    assert len(mot) == 1 and g >= 0 and z["gt_xy"][g, 0] == z["dt_xyz"][mot[0], 0] + 0.25 and z["gt_xy"][g + 1, 0] == z["dt_xyz"][mot[0], 0] - 0.25
    sc = z["dt_score"]
    assert len(set(sc.tolist())) == 7 and len({(a, b) for a, b in zip(z["dt_sample"], sc)}) < len(sc)        # ties inside and across samples
    assert (np.array([len(r["translation"]) for r in s["gt_records"]]) == 3).all() and len(z["gt_yaw"]) < len(s["gt_records"])   # the filter dropped some
    assert len(sc) < int(s["count"].sum())


def test_contract_tables_equal_the_host_evaluator_bit_for_bit():
    ev, got = _host(), _contract()
    assert set(got) == set(ev.tables)
    for name, a in got.items():
        b = np.asarray(ev.tables[name])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    sm = ev.summarize()
    assert 0.05 < sm["mean_ap"] < 0.9 and 0.1 < sm["nd_score"] < 0.9 and ((ev.tables["precision"] > 0) & (ev.tables["precision"] < 1)).any()


def test_interp_rule_equals_np_interp():
    rng = np.random.default_rng(2)
    for n in (1, 2, 5, 40):
        xp = np.sort(rng.integers(0, 12, n) / 8.0)                                # repeated abscissae
        fp = rng.normal(size=n)
        if n == 5:
            fp[1], fp[2] = np.inf, np.inf                                         # numpy's NaN fall-backs
        xs = np.concatenate([xp, rng.uniform(-0.5, 2, 50), [xp[0] - 1, xp[-1] + 1]])
        for right in (None, 0.0):
            want = np.interp(xs, xp, fp, right=right)
            got = np.array([nc.interp1(float(x), xp.tolist(), fp.tolist(), right) for x in xs])
            assert got.tobytes() == want.tobytes(), (n, right)


def test_rows_contract_equals_dets_to_nusc_and_pack_nusc():
    """rows_sample against the host path it restates: cells, ranks, source rows and every polynomial column on its bits; dt_quat and
    dt_yaw (math's sin, cos and atan2 against numpy's) inside the contract's interval"""
    s, ev = nc.test_set(), _host()
    z = ev.z
    mv, st = ne.attr_tables(nc.CLASSES)
    rng_ = [ne.DETECTION_CVPR_2019["class_range"][n] for n in nc.CLASSES]
    at = 0
    for i in (0, 4, 5, 10):
        got = nc.rows_sample(s["dets"][i], s["count"][i], s["poses"][i], list(range(nc.KC)), rng_, mv, st, nc.KC)
        cells = slice(i * nc.KC, (i + 1) * nc.KC)
        n, at = int(got["cnt"].sum()), int(z["dt_beg"][i * nc.KC])
        assert got["cnt"].tolist() == z["dt_cnt"][cells].tolist() and (got["beg"] + at).tolist() == z["dt_beg"][cells].tolist()
        for name in ("xyz", "size", "vel", "score", "cat", "attr", "rank"):
            assert np.asarray(got[name][:n], z["dt_" + name].dtype).tobytes() == z["dt_" + name][at:at + n].tobytes(), (i, name)
        assert (np.abs(got["quat"][:n] - z["dt_quat"][at:at + n]) <= got["quat_bound"][:n]).all()
        assert (np.abs(got["yaw"][:n] - z["dt_yaw"][at:at + n]) <= got["yaw_bound"][:n]).all()
        before = int(s["count"][:i].sum())
        assert (got["src"][:n] + before == z["dt_gidx"][at:at + n]).all() and (got["cat"][n:] == nc.KC).all() and (got["src"][n:] == -1).all()
        assert (got["quat_bound"][:n, 0] > 0).all() and (got["quat_bound"][:n] < 1e-14).all() and (got["yaw_bound"][:n] < 1e-13).all()


def test_category_order_is_the_walking_order():
    ev = _host()
    s = nc.test_set()
    p = ne.pack_nusc(s["gt_records"], s["ego"], nc.CLASSES, device="cpu", dt_records=s["dt_records"])
    order, cat_off = (t.numpy() for t in p.category_order())
    assert np.array_equal(order, ev.tables["order"]) and np.array_equal(cat_off, ev.tables["cat_off"])
    for name, a in p.numpy().items():
        assert np.array_equal(a, ev.z[name], equal_nan=True), name


@pytest.mark.parametrize("defect", nc.DEFECTS)
def test_each_planted_defect_changes_the_tables(defect):
    good, bad = _contract(), _contract(defect)
    changed = [n for n in good if not np.array_equal(good[n], bad[n], equal_nan=True)]
    assert changed, f"the test set does not see {defect}: strengthen it"
    assert {"precision", "confidence", "tp_err"} & set(changed) or defect == "last_gt_on_tie", (defect, changed)


def test_summarize_on_a_hand_computed_two_class_case():
    """car: two ground truths, three predictions (0.9 hits at 0.3 m, 0.8 misses, 0.7 hits at 1.5 m); barrier: one ground truth hit at
    0 m by its only prediction.  Worked by hand from the protocol."""
    q0 = [1.0, 0.0, 0.0, 0.0]
    gt = lambda x, name, attr: dict(sample_token=0, translation=[x, 0.0, 0.0], size=[2.0, 4.0, 1.5], rotation=q0, velocity=[1.0, 0.0], detection_name=name,
                                    attribute_name=attr, num_pts=3)
    dt = lambda x, sc, name, attr, size=(2.0, 4.0, 1.5): dict(sample_token=0, translation=[x, 0.0, 0.0], size=list(size), rotation=q0, velocity=[1.0, 0.0],
                                                              detection_name=name, detection_score=sc, attribute_name=attr)
    gts = [gt(0.0, "car", "vehicle.moving"), gt(10.0, "car", "vehicle.parked"), gt(20.0, "barrier", "")]
    dts = [dt(0.3, 0.9, "car", "vehicle.moving"), dt(30.0, 0.8, "car", "vehicle.moving"), dt(11.5, 0.7, "car", "vehicle.moving", (2.0, 4.0, 3.0)),
           dt(20.0, 0.6, "barrier", "cycle.with_rider")]
    ev = ne.NuscDetectionEval(gts, dts, [(0.0, 0.0, 0.0)], ["car", "barrier"]).evaluate()
    sm = ev.summarize()
    # car at 0.5 m: tp = 1, 1, 1 of npos 2 -> recall 0.5, 0.5, 0.5 and precision 1, 1/2, 1/3; interp takes the last of equal abscissae: at
    # recall <= 0.5 the line from (0.5, 1/3) ... so precision is 1/3 up to 0.5 and 0 beyond it
    want05 = np.where(REC < 0.5, 1.0, np.where(REC == 0.5, 1 / 3, 0.0))
    assert np.array_equal(ev.tables["precision"][0, 0], np.interp(REC, [0.5, 0.5, 0.5], [1.0, 0.5, 1 / 3], right=0)) and np.allclose(ev.tables["precision"][0, 0], want05)
    ap05 = np.mean(np.clip(want05[11:] - 0.1, 0, None)) / 0.9
    assert sm["label_aps"]["car"][0.5] == pytest.approx(ap05, abs=1e-15)
    # car at 2 m and 4 m: tp = 1, 1, 2 -> recall 0.5, 0.5, 1 and precision 1, 1/2, 2/3: 1 below 0.5, then the line from (0.5, 1/2) to (1, 2/3)
    want2 = np.where(REC < 0.5, 1.0, 0.5 + (REC - 0.5) * ((2 / 3 - 0.5) / 0.5))
    assert np.allclose(ev.tables["precision"][0, 2], want2, atol=1e-15) and np.array_equal(ev.tables["precision"][0, 3], ev.tables["precision"][0, 2])
    assert sm["label_aps"]["car"][2.0] == pytest.approx(np.mean(want2[11:] - 0.1) / 0.9, abs=1e-15)
    assert list(sm["label_aps"]["barrier"]) == [0.5, 1.0, 2.0, 4.0] and sm["mean_dist_aps"]["barrier"] == pytest.approx(1.0, abs=1e-15)      # mean(0.9 ..) / 0.9
    assert ev.tables["n_match"].tolist() == [[1, 1, 2, 2], [1, 1, 1, 1]] and ev.tables["n_gt"].tolist() == [2, 1]
    # the errors of the two car matches at 2 m: trans 0.3 and 1.5, scale 0 and 1 - 12 / 24, attr 0 and 1 (parked against moving)
    e = ev.tables["err"][ev.tables["dtm"][2] >= 0]
    assert np.allclose(e[:2, 0], [0.3, 1.5], atol=1e-15) and e[:2, 1].tolist() == [0.0, 0.5] and e[:2, 4].tolist() == [0.0, 1.0] and (e[:, 2:4] == 0).all()
    # confidence: 0.9 below recall 0.5, then the line 0.8 -> 0.7; the running means (0.3, 0.9) interpolated at it: 0.3 where the confidence is
    # 0.9 or more, 0.9 at 0.7; the TP metric is the mean over recall 0.11 .. 1
    conf = np.where(REC < 0.5, 0.9, 0.8 - (REC - 0.5) * 0.2)
    assert np.allclose(ev.tables["confidence"][0, 2], conf, atol=1e-15)
    trans = np.interp(conf[::-1], [0.7, 0.9], [0.9, 0.3])[::-1]
    assert sm["label_tp_errors"]["car"]["trans_err"] == pytest.approx(np.mean(trans[11:]), abs=1e-14)
    assert sm["label_tp_errors"]["barrier"]["trans_err"] == 0.0 and np.isnan(sm["label_tp_errors"]["barrier"]["attr_err"])
    assert np.isnan(sm["label_tp_errors"]["barrier"]["vel_err"]) and sm["label_tp_errors"]["barrier"]["orient_err"] == 0.0
    mean_ap = np.mean([np.mean(list(sm["label_aps"][n].values())) for n in ("car", "barrier")])
    assert sm["mean_ap"] == pytest.approx(mean_ap, abs=1e-15)
    errs = {m: np.nanmean([sm["label_tp_errors"][n][m] for n in ("car", "barrier")]) for m in ne.TP_METRICS}
    assert sm["nd_score"] == pytest.approx((5 * mean_ap + sum(max(1 - v, 0) for v in errs.values())) / 10, abs=1e-15)
    assert sm["tp_errors"]["vel_err"] == sm["label_tp_errors"]["car"]["vel_err"] == 0.0


def test_attribute_rule_for_every_class_moving_and_still():
    """the table of nuscenes.py:258-291, written from the source lines: (class, speed > 0.2) -> attribute"""
    want = {"car": ("vehicle.moving", "vehicle.parked"), "truck": ("vehicle.moving", "vehicle.parked"), "construction_vehicle": ("vehicle.moving", "vehicle.parked"),
            "bus": ("vehicle.moving", "vehicle.stopped"), "trailer": ("vehicle.moving", "vehicle.parked"), "barrier": ("cycle.with_rider", "cycle.with_rider"),
            "motorcycle": ("cycle.with_rider", "cycle.without_rider"), "bicycle": ("cycle.with_rider", "cycle.without_rider"),
            "pedestrian": ("pedestrian.moving", "pedestrian.standing"), "traffic_cone": ("cycle.with_rider", "cycle.with_rider")}
    mv, st = ne.attr_tables(nc.CLASSES)
    pose = np.array([[1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]], np.float64)
    for k, name in enumerate(nc.CLASSES):
        assert (ne.ATTRIBUTES[mv[k]], ne.ATTRIBUTES[st[k]]) == want[name], name
        for vx, which in ((0.25, 0), (0.125, 1), (0.2, 1)):                         # 0.2 itself is not moving (float32 0.2 is above it: use the float64 rule on 0.125)
            if vx == 0.2:
                continue
            d = np.zeros((1, 1, 11), np.float32)
            d[0, 0] = [1, 2, 0, 1, 1, 1, vx, 0, 0.3, 0.5, k]
            rec = ne.dets_to_nusc(d, [1], pose, nc.CLASSES)[0]
            assert rec["attribute_name"] == want[name][which] and rec["detection_name"] == name
