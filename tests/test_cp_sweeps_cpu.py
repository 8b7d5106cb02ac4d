"""CPU: the CenterPoint multi-sweep input without a GPU -- the ABI of include/minddet_hip_cpsweeps.h (the function exported,
the semantic refusals answered before any device call, the ctypes mirror laid out as the header says), the
contract tests/cp_sweeps_contract.py against the reference's own outputs (tests/golden/cp_sweeps_vectors.npz, written by
tests/golden/gen_cp_sweeps.py from LoadPointCloudFromFile and read_sweep), det_ops.SweepMerger's tables against the recorded draw,
det_ops.SweepRing's host matrices, the two configs and the refused options."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from minddet_amd import _lib, det_ops
from tests import cp_sweeps_contract as sc
from tests import abi_header as ah
from tests.abi_cases import I
from tests.abi_cases_cpsweeps import CASES, F64, CPSweeps
from tests.abi_derive import attr, both, edited, lib_handle, rc, refuse_single_defects, shape
from tests.cp_sweeps_cases import GOLD, NAMES, case_tables, contract_case, fixture_case, pose, radius, reference_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "md_cp_sweeps_merge"
U8 = "uint8"


def _hdr():
    return ah.header("minddet_hip_cpsweeps.h")


def test_header_declares_the_symbol_and_the_library_exports_it():
    hdr = _hdr()
    assert ah.aot_symbols(hdr) == [SYM] and '#include "minddet_hip_points.h"' in hdr
    for cite in ("loading.py:56-80, 133-159", "multi_sweep_inference_ros.py:194-270", "nusc_common.py:443-450", "shuffle_points", "Waymo", "virtual",
                 "quaternions"):
        assert cite in hdr, cite
    assert "minddet_hip_cpsweeps.h" in open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    assert {c.sym for c in CASES} == {SYM} and len({c.id for c in CASES}) == len(CASES)
    assert getattr(lib_handle(), SYM)(0, None, None, None, None, None, None) == 1      # wrong parameter count, before anything else
    assert SYM not in _lib.exported_symbols()                                            # declared in the new header only


def test_ctypes_mirror_limits_and_workspace_have_the_headers_layout():
    hdr = _hdr()
    assert ah.statements("md_cp_sweeps_attrs", hdr) == ["float radius", "int32_t reserved0"]
    for got in (det_ops._CPSweepsAttrs, CPSweeps):
        assert C.sizeof(got) == 8 and got.radius.offset == 0 and got.radius.size == 4 and got.reserved0.offset == 4 and got.reserved0.size == 4
    for name, macro in (("CPSWEEPS_MAX_SWEEPS", "MD_CPSWEEPS_MAX_SWEEPS"), ("CPSWEEPS_MAX_BATCH", "MD_CPSWEEPS_MAX_BATCH")):
        assert getattr(det_ops, name) == ah.defines(hdr)[macro]
    assert det_ops.CPSWEEPS_MAX_SWEEPS >= 16 and det_ops.CPSWEEPS_MAX_BATCH >= 256
    assert (det_ops.SWEEP_REMOVE_CLOSE, det_ops.SWEEP_TRANSFORM) == (sc.REMOVE_CLOSE, sc.TRANSFORM) == (1, 2)
    assert "4 (N / 256 + B S + 3) bytes" in hdr
    assert det_ops.cp_sweeps_merge_workspace_bytes(300, 2, 3) == 36 <= 40 and det_ops.cp_sweeps_merge_workspace_bytes(1040000, 4, 10) == 16416 <= 16420


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_cpsweeps", case)


def test_semantic_refusals_return_the_documented_codes():
    ARG, SIZE = 2, 4
    ws, pool = CASES
    for i, e in enumerate([shape(0, (300, 3)), shape(0, (300, 6)), shape(1, (2, 3, 3), I), shape(1, (3, 3, 2), I), shape(1, (2, 4, 2), I),
                           shape(2, (2, 3, 9), F64), shape(2, (2, 4, 12), F64), shape(3, (2, 4), F64), shape(3, (3, 3), F64), shape(4, (2, 4), I),
                           shape(5, (299, 5)), shape(5, (300, 4)), shape(5, (300, 6)), shape(6, (2,), I), shape(6, (4,), I), shape(7, (3,), I)]):
        assert rc(ws, e) == ARG, i
    assert rc(pool, shape(5, (299, 5))) == ARG              # M < N
    nan, inf = float("nan"), float("inf")
    for v in (nan, inf, -inf, -1.0, -1e-30):
        assert rc(ws, attr("radius", v)) == ARG, v
    assert rc(ws, attr("reserved0", 1)) == ARG
    S1, B1 = det_ops.CPSWEEPS_MAX_SWEEPS + 1, det_ops.CPSWEEPS_MAX_BATCH + 1
    grow_s = both(shape(1, (2, S1, 2), I), shape(2, (2, S1, 12), F64), shape(3, (2, S1), F64), shape(4, (2, S1), I))
    assert rc(pool, grow_s) == SIZE
    grow_b = both(shape(1, (B1, 3, 2), I), shape(2, (B1, 3, 12), F64), shape(3, (B1, 3), F64), shape(4, (B1, 3), I), shape(6, (B1 + 1,), I),
                   shape(7, (B1,), I))
    assert rc(pool, grow_b) == SIZE
    call = edited(pool, lambda c: None)                       # (the shapes alone say 2^30 points: the host blocks stay small, nothing is touched)
    call.shapes[0], call.shapes[5] = [1 << 30, 4], [1 << 30, 5]
    assert call.run(lib_handle()) == SIZE
    assert rc(ws, shape(8, (35,), U8)) == SIZE              # 36 bytes are used


def test_aliased_outputs_are_refused():
    """an output at the address of an input or of another output: rc 2 before any device call"""
    lib = lib_handle()
    case = CASES[0]
    for out, other in ((5, 0), (6, 1), (7, 4), (7, 6), (6, 5)):
        call = edited(case, lambda c: None)
        n, ops = call.n, call.case.operands
        bufs = [(C.c_char * 65536)() for _ in range(n)]
        params = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
        params[out] = params[other]
        ndims = (C.c_int * n)(*[len(t.shape) for t in ops])
        keep = [(C.c_int64 * max(len(t.shape), 1))(*t.shape) for t in ops]
        shapes = (C.POINTER(C.c_int64) * n)(*[C.cast(k, C.POINTER(C.c_int64)) for k in keep])
        dtypes = (C.c_char_p * n)(*[t.dtype.encode() for t in ops])
        assert getattr(lib, case.sym)(n, params, ndims, shapes, dtypes, None, C.byref(case.extra)) == 2, (out, other)


def test_fixture_carries_what_the_cases_promise():
    z = np.load(GOLD)
    assert sorted(z["cases"]) == sorted(NAMES) and os.path.getsize(GOLD) < 100 * 1000 and radius() == 1.0
    small, pad, batch, plants = (fixture_case(n) for n in NAMES)
    assert len(small) == 1 and len(small[0]["lengths"]) == 3 and small[0]["lengths"].min() >= 150 and small[0]["has_matrix"].tolist() == [False, True, True]
    p = pad[0]
    assert len(pad) == 1 and p["has_matrix"].tolist() == [False, True, False, False] and p["time_lags"][2:].tolist() == [0.0, 0.0]
    assert sorted(p["seg_flags"].tolist()) == [0, 1, 1, 3]                                     # quirk (b): a padding sweep is still filtered
    assert len(batch) == 2 and batch[0]["order"].tolist() != batch[1]["order"].tolist()
    q = plants[0]
    assert q["plant_kept"].sum() not in (0, len(q["plant_kept"])) and np.isnan(q["points"][:, :2]).any() and np.signbit(q["points"][:, 0][q["points"][:, 0] == 0]).any()
    r = np.float32(1)
    xs = np.abs(q["points"][:, :2])
    assert (xs == r).any() and (xs == np.nextafter(r, np.float32(0))).any() and (xs == np.nextafter(r, np.float32(2))).any()
    for name in NAMES:
        for s in fixture_case(name):
            assert s["points"].dtype == s["combined"].dtype == np.float32 and s["points"].shape[1] == 5 and s["matrices"].dtype == np.float64
            assert s["seg_flags"][0] == 0 and len(s["points"]) == s["lengths"].sum() > len(s["combined"])      # (something is dropped in every sample)
            assert sorted(s["order"].tolist()) == list(range(len(s["lengths"]) - 1))


@pytest.mark.parametrize("name", NAMES)
def test_contract_equals_the_reference(name):
    """exact parts exact, xyz within the condition, and the reference itself holds the cap"""
    c = contract_case(name)
    ref, offs = reference_cloud(name)
    assert c["status"].tolist() == [0] * len(fixture_case(name)) and np.array_equal(c["offsets"], offs)
    full = np.zeros_like(c["points"])
    full[:len(ref)] = ref
    differ, total = sc.check(full, offs, c, what=name)
    assert total > 0 and differ <= sc.FEW * total
    if name == "plants":
        s = fixture_case(name)[0]
        n, n_key = len(s["plant_kept"]), int(s["lengths"][0])
        kept_rows = set(c["src"].tolist())
        assert set(range(n_key)) <= kept_rows                                                      # quirk (a): the key frame is not filtered
        starts = np.concatenate([[0], np.cumsum(s["lengths"])])
        assert [(int(starts[1]) + i) in kept_rows for i in range(n)] == s["plant_kept"].tolist()    # the transformed sweep's plants lead its frame
        assert [(int(starts[3]) - n + i) in kept_rows for i in range(n)] == s["plant_kept"].tolist()      # the padding sweep's plants end its frame
        row = int(np.flatnonzero(c["src"] == int(s["cancel_row"]))[0])
        assert c["lo"][row, 0] != c["hi"][row, 0] and c["lo"][row, 0] <= c["points"][row, 0] <= c["hi"][row, 0]      # the interval branch is a real interval here


def test_contract_interval_and_decisions_on_hand_made_rows():
    m = np.array([1.0, 0, 0, -5.0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])
    v, e = sc.transform(m, np.array([[5.0, 2.0, 3.0]], np.float32))
    assert v.tolist() == [[0.0, 2.0, 3.0]] and e[0, 0] == 4 * sc.U * 10 and e[0, 1] == 4 * sc.U * 2
    rows = np.array([[1, 0], [0.5, 0.5], [np.nan, 0], [-0.0, 0.0], [0.5, -1]], np.float32)
    assert sc.keep_mask(rows, 1.0).tolist() == [True, False, True, False, True]
    pts = np.zeros((4, 4), np.float32)
    seg = np.array([[[0, 2], [2, 5]], [[3, 4], [0, 0]]])
    c = sc.merge(pts, seg, np.zeros((2, 2, 12)), np.zeros((2, 2)), np.zeros((2, 2), np.int32), 1.0)
    assert c["status"].tolist() == [1, 0] and c["offsets"].tolist() == [0, 0, 1]
    seg = np.array([[[0, 4], [0, 1]]])
    c = sc.merge(pts, seg, np.zeros((1, 2, 12)), np.zeros((1, 2)), np.zeros((1, 2), np.int32), 1.0, M=6)
    assert c["status"].tolist() == [2] and c["offsets"].tolist() == [0, 0] and c["points"].shape == (6, 5)


@pytest.mark.parametrize("name", NAMES)
def test_merger_tables_reproduce_the_fixture_from_the_recorded_draw(name):
    ss = fixture_case(name)
    merger = det_ops.SweepMerger(len(ss[0]["lengths"]), min_distance=radius())
    args = ([s["lengths"].tolist() for s in ss], [[m if h else None for m, h in zip(s["matrices"], s["has_matrix"])] for s in ss],
            [s["time_lags"].tolist() for s in ss])
    t = merger.tables(*args, order=[s["order"] for s in ss])
    want = case_tables(name)
    for k in ("seg_range", "transforms", "time_lag", "seg_flags"):
        assert t[k].dtype == want[k].dtype and np.array_equal(t[k], want[k]), k
    # the loader's own draw: np.random.choice(n, n, replace=False) right after the seed
    for b, s in enumerate(ss):
        one = merger.tables(args[0][b], args[1][b], args[2][b], order=np.random.RandomState(int(s["seed"])))
        assert one["order"].tolist() == [s["order"].tolist()] and np.array_equal(one["seg_flags"][0], s["seg_flags"])
    plain = merger.tables(*args)
    assert plain["order"].tolist() == [list(range(len(ss[0]["lengths"]) - 1))] * len(ss)


def test_merger_demo_order_and_ring_matrices():
    rng = np.random.default_rng(4)
    demo = det_ops.SweepMerger(4, min_distance=None, order="oldest_first")
    mats = [None] + [pose(rng) for _ in range(3)]
    t = demo.tables([10, 20, 30, 40], mats, [0.0, 0.1, 0.2, 0.3])
    assert t["seg_range"][0].tolist() == [[60, 100], [30, 60], [10, 30], [0, 10]] and t["seg_flags"][0].tolist() == [2, 2, 2, 0]
    assert t["time_lag"][0].tolist() == [0.3, 0.2, 0.1, 0.0] and np.array_equal(t["transforms"][0, 0], mats[3][:3].reshape(12))
    assert demo.radius == 0.0 and det_ops.SweepMerger(4, min_distance=0.5, order="oldest_first").tables([1] * 4, mats, [0] * 4)["seg_flags"][0].tolist() == [3, 3, 3, 0]
    ring = det_ops.SweepRing(3, 50, device="cpu")
    poses = [pose(rng, 30.0) for _ in range(5)]
    for i, g in enumerate(poses):
        assert ring.admit(40 + i, g, 10.0 + 0.05 * i) == i % 3
        held = poses[max(0, i - 2):i + 1]
        got = ring.matrices()
        assert len(got) == len(held)
        for m, gi in zip(got, held):
            assert np.abs(m - np.linalg.inv(g) @ gi).max() <= 1e-15 * max(1.0, np.abs(m).max())
    t = ring.tables()                                         # frames 2, 3, 4 in slots 2, 0, 1; oldest first, the current frame last
    assert t["seg_range"][0].tolist() == [[100, 142], [0, 43], [50, 94]] and t["seg_flags"][0].tolist() == [2, 2, 0]
    assert np.allclose(t["time_lag"][0], [0.1, 0.05, 0.0], atol=1e-12) and t["time_lag"][0, 2] == 0.0
    with pytest.raises(ValueError):
        ring.admit(51, poses[0], 11.0)
    early = det_ops.SweepRing(3, 50, order="key_first", min_distance=1.0, device="cpu")
    early.admit(7, poses[0], 1.0)
    t = early.tables()
    assert t["seg_range"][0].tolist() == [[0, 7], [0, 0], [0, 0]] and t["seg_flags"][0, 0] == 0


def test_configs_load_and_build_their_ops():
    from minddet.models import Config, build_detector

    nusc = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc_sweeps.py"))
    base = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc_points.py"))
    assert dict(nusc.data["sweeps"]) == dict(nsweeps=10, min_distance=1.0, order="key_first") == dict(nusc.model["sweeps"])
    assert {k: v for k, v in dict(nusc.model).items() if k != "sweeps"} == dict(base.model) and nusc.test_cfg == base.test_cfg
    m = det_ops.SweepMerger.from_config(nusc)
    assert (m.nsweeps, m.min_distance, m.order) == (10, 1.0, "key_first")
    tiny = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_tiny_sweeps.py"))
    tbase = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_tiny_points_train.py"))
    assert {k: v for k, v in dict(tiny.model).items() if k != "sweeps"} == dict(tbase.model) and tiny.train_cfg == tbase.train_cfg
    det = build_detector(dict(tiny.model), dict(tiny.train_cfg), tiny.test_cfg)
    op = det.sweeps_op()
    assert (op.nsweeps, op.min_distance, op.order) == (3, 1.0, "key_first") and det.sweeps_op() is op
    assert det_ops.SweepMerger.from_config(tiny).nsweeps == 3 and det.augment_op().min_points_in_gt == 2
    with pytest.raises(ValueError):                           # a model without `sweeps`
        build_detector(dict(tbase.model), dict(tbase.train_cfg), tbase.test_cfg).sweeps_op()
    with pytest.raises(ValueError):
        det_ops.SweepMerger.from_config(tbase)


def test_refused_options_raise():
    for kw in (dict(virtual=True), dict(random_select=True), dict(dataset="WaymoDataset"), dict(order="random"), dict(no_such_option=1),
               dict(min_distance=-1.0), dict(min_distance=float("nan"))):
        with pytest.raises(ValueError):
            det_ops.SweepMerger(3, **kw)
    for n in (0, det_ops.CPSWEEPS_MAX_SWEEPS + 1):
        with pytest.raises(ValueError):
            det_ops.SweepMerger(n)
    assert det_ops.SweepMerger(3, virtual=False, random_select=False, dataset="NuScenesDataset").nsweeps == 3      # named but off: fine
    m = det_ops.SweepMerger(3)
    with pytest.raises(ValueError):                           # not a permutation
        m.tables([1, 2, 3], [None] * 3, [0.0] * 3, order=[0, 0])
    with pytest.raises(ValueError):                           # two frames for three sweeps
        m.tables([1, 2], [None] * 2, [0.0] * 2)
    with pytest.raises(ValueError):                           # a 3x4 where the 4x4 goes
        m.tables([1, 2, 3], [None, np.eye(4)[:3], None], [0.0] * 3)
    seg, tf, lag, fl = torch.zeros((1, 2, 2), dtype=torch.int32), torch.zeros((1, 2, 12), dtype=torch.float64), torch.zeros((1, 2), dtype=torch.float64), \
        torch.zeros((1, 2), dtype=torch.int32)
    for bad in (torch.zeros((4, 3)), torch.zeros((4, 6)), torch.zeros((4,))):      # points that are not 4 or 5 wide
        with pytest.raises(ValueError):
            det_ops.cp_sweeps_merge(bad, seg, tf, lag, fl)
    for args in ((seg, tf[:, :1], lag, fl), (seg, tf, lag[:, :1], fl), (seg, tf, lag, torch.zeros((2, 2), dtype=torch.int32)), (seg[..., :1], tf, lag, fl)):
        with pytest.raises(ValueError):                       # table shapes that disagree
            det_ops.cp_sweeps_merge(torch.zeros((4, 5)), *args)
    with pytest.raises(ValueError):                           # out with fewer rows than the pool
        det_ops.cp_sweeps_merge(torch.zeros((4, 5)), seg, tf, lag, fl, out=torch.zeros((3, 5)))
    with pytest.raises(ValueError):
        det_ops.SweepRing(3, 10, device="cpu").push(torch.zeros((11, 5)), np.eye(4), 0.0)
