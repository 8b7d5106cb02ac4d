"""-m gpu: md_assign_targets (csrc/targets.hip) against the reference's own create_target_np outputs and a plain per-anchor judge.

Conditions, fixed beforehand:
  labels, bbox_outside_weights, gt ids     bit for bit
  bbox_targets columns 0, 1, 2, 6          bit for bit (same float32 operation order as the reference, contraction off)
  bbox_targets columns 3, 4, 5 (log)       at most 4 fp32 ulp from the reference value, or 1e-7 absolute (device logf against numpy's log
                                           for target_vectors.npz and the car size, against the judge's float64 log for target_edges.npz)
  masked-out and non-positive anchors      label -1 (0 for background), targets +0.0, weight +0.0, gt id -1, exactly
  every element of all four outputs        written: they start as 0xFF bytes (and, the integers reading -1 under that fill, as 0x5A bytes)
  scratch forms, calls, streams, wrappers  identical bytes

References: tests/golden/target_vectors.npz (four random scenes, tests/golden/gen_targets.py), oracle/np_ops.py::create_target at the
PointPillars car size (107 136 anchors), and tests/golden/target_edges.npz (tests/golden/gen_target_edges.py): the planted edges, G = 1 /
255 / 256 / 257 / 1024, A = 1 / 255 / 256 / 257 / 587, with tests/targets_contract.py as the judge whose deliberate mistakes
tests/test_targets_cpu.py shows that fixture to catch."""
import os

import numpy as np
import pytest
import torch

from oracle import np_ops
from tests import targets_contract as tc
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "target_vectors.npz"))


def _check_targets(got, ref):
    np.testing.assert_array_equal(got[:, [0, 1, 2, 6]], ref[:, [0, 1, 2, 6]])
    a, b = got[:, 3:6], ref[:, 3:6]
    ulp = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    assert (ulp <= 4).all() or np.allclose(a, b, rtol=0, atol=1e-7), ulp.max()


def _run(anchors, gt, cls, mt, ut, mask):
    from minddet_amd import det_ops

    T = lambda x, dt=None: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    out = det_ops.assign_targets(T(anchors), T(gt), T(cls), T(mt), T(ut), None if mask is None else T(mask))
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("case", ["car", "nomask", "nogt", "pedcyc"])
def test_device_equals_reference_vectors(case):
    mask = G[case + "_mask"]
    labels, targets, weights, gt_ids = _run(G[case + "_anchors"], G[case + "_gt"], G[case + "_cls"], G[case + "_mt"], G[case + "_ut"],
                                            mask if mask.size else None)
    np.testing.assert_array_equal(labels, G[case + "_labels"])
    np.testing.assert_array_equal(weights, G[case + "_weights"])
    _check_targets(targets, G[case + "_targets"])
    assert ((gt_ids >= 0) == (labels > 0)).all()
    want = np_ops.create_target(G[case + "_anchors"], G[case + "_gt"], G[case + "_cls"], G[case + "_mt"], G[case + "_ut"],
                                mask.astype(bool) if mask.size else None)
    np.testing.assert_array_equal(want[0], G[case + "_labels"])          # the oracle is pinned to these vectors (test_targets_cpu.py)
    np.testing.assert_array_equal(gt_ids, want[3])


def test_pointpillars_car_size_vs_oracle():
    anchors = np_ops.create_anchors_3d_stride((1, 248, 216), sizes=(1.6, 3.9, 1.56), anchor_strides=(0.32, 0.32, 0.0),
                                              anchor_offsets=(0.16, -39.52, -1.78), rotations=(0, 1.57)).reshape(-1, 7).astype(np.float32)
    assert anchors.shape[0] == 107136
    rng = np.random.default_rng(5)
    gt = np.zeros((23, 7), np.float32)
    gt[:, 0] = rng.uniform(0, 69.12, 23); gt[:, 1] = rng.uniform(-39.68, 39.68, 23); gt[:, 2] = rng.uniform(-2, 0, 23)
    gt[:, 3] = rng.uniform(1.4, 1.9, 23); gt[:, 4] = rng.uniform(3.2, 4.6, 23); gt[:, 5] = rng.uniform(1.3, 1.8, 23)
    gt[:, 6] = rng.uniform(-np.pi, np.pi, 23)
    mask = (rng.uniform(0, 1, anchors.shape[0]) < 0.2).astype(np.uint8)
    mt = np.full((anchors.shape[0],), 0.6, np.float32)
    ut = np.full((anchors.shape[0],), 0.45, np.float32)
    cls = np.ones((23,), np.int32)
    labels, targets, weights, gt_ids = _run(anchors, gt, cls, mt, ut, mask)
    rl, rt, rw, rg = np_ops.create_target(anchors, gt, cls, mt, ut, mask.astype(bool))
    np.testing.assert_array_equal(labels, rl)
    np.testing.assert_array_equal(weights, rw)
    np.testing.assert_array_equal(gt_ids, rg)
    _check_targets(targets, rt)
    assert (labels > 0).sum() > 20


# ------------------------------------------------------------------ the edge fixture: raw calls into garbage-filled outputs
_dev, _judged = {}, {}


def _inputs(case):
    """the six input operands of a fixture case on the device (gt / cls: None for an empty list), uploaded once"""
    if case not in _dev:
        c = tc.cases()[case]
        T = lambda x: torch.from_numpy(np.array(x)).to(DEV)          # a copy: the fixture's arrays are read-only
        g = c["gt"].shape[0]
        _dev[case] = [T(c["anchors"]), T(c["gt"]) if g else None, T(c["cls"]) if g else None, T(c["mt"]), T(c["ut"]), T(c["mask"])]
    return _dev[case]


def _judge(case):
    if case not in _judged:
        c = tc.cases()[case]
        _judged[case] = tc.judge(*(c[k] for k in tc.FIELDS))
    return _judged[case]


def _raw(ins, fill=0xFF, ws=None, stream=None):
    """md_assign_targets on device operands `ins` with all four outputs pre-filled with `fill` bytes -> (labels, targets, weights, gt_ids)
    as numpy"""
    from minddet_amd import _lib

    A = ins[0].shape[0]
    buf = lambda n, dt: torch.full((n * 4,), fill, dtype=torch.uint8, device=DEV).view(dt)
    outs = [buf(A, torch.int32), buf(A * 7, torch.float32).view(A, 7), buf(A, torch.float32), buf(A, torch.int32)]
    ops = list(ins) + outs + ([ws] if ws is not None else [])
    if stream is None:
        _lib.call("md_assign_targets", ops)
    else:
        stream.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(stream):
            _lib.call("md_assign_targets", ops)
        stream.synchronize()
    return [o.cpu().numpy() for o in outs]


def _same_bytes(a, b, what):
    for x, y, name in zip(a, b, ("labels", "bbox_targets", "bbox_outside_weights", "gt_ids")):
        assert x.tobytes() == y.tobytes(), "%s: %s differs" % (what, name)


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _check_case(case, got, want=None, judged=None):
    """the module's conditions on one device result; want: dict with labels / targets / weights / gt_ids, judged: the judge's four"""
    c = tc.cases()[case] if want is None else want
    jl, jt, jw, jg = _judge(case) if judged is None else judged
    labels, targets, weights, gt_ids = got
    np.testing.assert_array_equal(labels, c["labels"])
    np.testing.assert_array_equal(_u32(weights), _u32(c["weights"]))
    np.testing.assert_array_equal(gt_ids, c["gt_ids"])
    np.testing.assert_array_equal(_u32(targets[:, [0, 1, 2, 6]]), _u32(c["targets"][:, [0, 1, 2, 6]]))
    np.testing.assert_array_equal(labels, jl)
    np.testing.assert_array_equal(gt_ids, jg)
    np.testing.assert_array_equal(_u32(targets[:, [0, 1, 2, 6]]), _u32(jt[:, [0, 1, 2, 6]].astype(np.float32)))
    ulp, err = tc.log_ulps(targets[:, 3:6], jt[:, 3:6])
    print("%s: worst log distance %d fp32 ulp, %.3g absolute, over %d positive anchors" % (case, ulp.max(), err.max(), (labels > 0).sum()))
    assert (ulp <= 4).all() or (err <= 1e-7).all(), (ulp.max(), err.max())
    off = labels <= 0
    assert (_u32(targets[off]) == 0).all() and (_u32(weights[off]) == 0).all() and (gt_ids[off] == -1).all(), "a non-positive anchor carries a target"
    assert (labels[c["mask"] == 0] == -1).all(), "a masked-out anchor has a label"
    assert (_u32(weights[~off]) == 0x3F800000).all()
    assert not (_u32(targets) == 0xFFFFFFFF).any() and not (_u32(weights) == 0xFFFFFFFF).any(), "an element of a float output was not written"


@pytest.mark.parametrize("case", tc.case_names())
def test_device_equals_reference_edges(case):
    got = _raw(_inputs(case))
    _check_case(case, got)
    # -1 is what 0xFF bytes read as in labels and gt_ids: a second fill shows an integer the kernel skipped
    _same_bytes(got, _raw(_inputs(case), fill=0x5A), case + " with outputs pre-filled 0x5A")


def test_planted_edges_by_name():
    c = tc.cases()["planted"]
    labels, targets, weights, gt_ids = _raw(_inputs("planted"))
    for name, rows in tc.edges().items():
        for a, lab, gid in rows:
            assert (labels[a], gt_ids[a]) == (lab, gid), "%s (anchor %d: label %d id %d, reference %d / %d)" % (
                tc.EDGE_MESSAGES[name], a, labels[a], gt_ids[a], lab, gid)
    far = tc.fixture()["planted_far_boxes"]
    assert not np.isin(gt_ids, far).any(), "a box nothing overlaps forced an anchor"
    untouched = (c["labels"] == 0) & (c["mask"] != 0)
    assert (labels[untouched] == 0).all(), "an anchor no box overlaps is not background"
    a = int(tc.edges()["on_anchor"][0, 0])
    assert (_u32(targets[a]) == 0).all() and weights[a] == 1, "a box on its anchor encodes to something else than +0.0"
    tied = tc.edges()["tied_anchors"][:, 0]
    assert len(set(gt_ids[tied])) == 1 and (labels[tied] > 0).all(), tc.EDGE_MESSAGES["tied_anchors"]


@pytest.mark.parametrize("case", ["planted", "g1024"])
def test_colmax_scratch_forms_agree(case):
    """the per-box column maxima are accumulated by atomicMax into scratch that md_assign_targets clears itself: a caller workspace
    of exactly 4 G bytes full of 0xFF, a clean one, and the library's pool right after a call with G = 1024 give identical bytes"""
    ins = _inputs(case)
    g = ins[1].shape[0]
    dirty = _raw(ins, ws=torch.full((4 * g,), 0xFF, dtype=torch.uint8, device=DEV))
    clean = _raw(ins, ws=torch.zeros((4 * g,), dtype=torch.uint8, device=DEV))
    _raw(_inputs("g1024"))
    pooled = _raw(ins)
    np.testing.assert_array_equal(dirty[0], tc.cases()[case]["labels"])
    np.testing.assert_array_equal(dirty[3], tc.cases()[case]["gt_ids"])
    _same_bytes(dirty, clean, case + ": 0xFF workspace against clean workspace")
    _same_bytes(dirty, pooled, case + ": 0xFF workspace against the pool after G = 1024")


@pytest.mark.parametrize("case", ["planted", "g1024", "a_ragged"])
def test_bit_identical_across_calls_and_streams(case):
    ins = _inputs(case)
    first = _raw(ins)
    for i in range(2):
        _same_bytes(first, _raw(ins), "%s: call %d" % (case, i + 2))
    _same_bytes(first, _raw(ins, stream=torch.cuda.Stream(device=DEV)), case + ": second stream")


def test_wrappers_equal_raw_calls():
    """det_ops.assign_targets and assign_targets_batch (B = 2: `planted` under two masks) against the raw calls, byte for byte"""
    from minddet_amd import det_ops

    c = tc.cases()["planted"]
    ins = _inputs("planted")
    mask2 = c["mask"].copy()
    mask2[tc.edges()["masked_best"][0, 0]] = 1                 # the best anchor is back ...
    mask2[tc.edges()["tied_anchors"][:2, 0]] = 0               # ... and two of the four tied anchors are gone
    m2 = torch.from_numpy(mask2).to(DEV)
    raw = [_raw(ins), _raw(ins[:5] + [m2])]
    _check_case("planted", raw[0])
    want2 = tc.judge(c["anchors"], c["gt"], c["cls"], c["mt"], c["ut"], mask2)
    _check_case("planted under the second mask", raw[1], judged=want2,
                want=dict(labels=want2[0], targets=want2[1].astype(np.float32), weights=want2[2], gt_ids=want2[3], mask=mask2))
    assert (raw[0][0] != raw[1][0]).any()
    one = [o.cpu().numpy() for o in det_ops.assign_targets(*ins)]
    _same_bytes(raw[0], one, "det_ops.assign_targets")
    batch = det_ops.assign_targets_batch(ins[0], [ins[1], ins[1]], [ins[2], ins[2]], ins[3], ins[4], torch.stack([ins[5], m2]))
    assert [tuple(t.shape) for t in batch] == [(2, 348), (2, 348, 7), (2, 348), (2, 348)]
    for b in range(2):
        _same_bytes(raw[b], [t[b].cpu().numpy() for t in batch], "det_ops.assign_targets_batch, sample %d" % b)


def _expect_empty(got, mask, what):
    labels, targets, weights, gt_ids = got
    inside = np.ones(labels.shape, bool) if mask is None else mask != 0
    assert (labels[inside] == 0).all() and (labels[~inside] == -1).all(), what + ": labels"
    assert (_u32(targets) == 0).all() and (_u32(weights) == 0).all() and (gt_ids == -1).all(), what + ": targets / weights / ids"


def test_no_ground_truth_with_a_mask():
    """G = 0: label 0 inside the mask, -1 outside, everything else +0.0 / -1 -- through the raw call with NULL operands"""
    ins = _inputs("nogt_masked")
    assert ins[1] is None and ins[2] is None
    mask = tc.cases()["nogt_masked"]["mask"]
    for fill in (0xFF, 0x5A):
        _expect_empty(_raw(ins, fill=fill), mask, "G = 0, fill %#x" % fill)


@pytest.mark.parametrize("masked", [True, False])
def test_empty_scenes_through_det_ops(masked):
    """a scene without ground truth, given as [0,7] / [0] tensors and as None, and a scene whose only box is the far padding box of
    graphs.PointPillars.train_example (classes given and defaulted): background inside the mask, nothing else.  (gt_boxes None, which
    assign_targets_batch documents, used to raise AttributeError in det_ops.assign_targets before the operator was reached.)"""
    from minddet_amd import det_ops

    a, _, _, mt, ut, m = _inputs("nogt_masked")
    mask = tc.cases()["nogt_masked"]["mask"] if masked else None
    m = m if masked else None
    run = lambda g, c: [o.cpu().numpy() for o in det_ops.assign_targets(a, g, c, mt, ut, m)]
    _expect_empty(run(torch.zeros((0, 7), device=DEV), torch.zeros((0,), dtype=torch.int32, device=DEV)), mask, "[0,7] boxes")
    _expect_empty(run(torch.zeros((0, 7), device=DEV), None), mask, "[0,7] boxes, no classes")
    _expect_empty(run(None, None), mask, "boxes None")
    far = torch.tensor([[1e6, 1e6, 0.0, 1.0, 1.0, 1.0, 0.0]], dtype=torch.float32, device=DEV)
    _expect_empty(run(far, torch.full((1,), 2, dtype=torch.int32, device=DEV)), mask, "the far box alone")
    _expect_empty(run(far, None), mask, "the far box alone, no classes")
    _expect_empty([o[0].cpu().numpy() for o in det_ops.assign_targets_batch(a, [None], None, mt, ut, None if m is None else m[None])], mask,
                  "assign_targets_batch, boxes None")
