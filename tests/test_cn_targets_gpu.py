"""-m gpu: md_cn_assign_targets (det_ops.cn_assign_targets / CenterNetTargets, csrc/cntargets.hip) against the reference's own
COCOHP.preprocess_fn outputs (tests/golden/cn_target_vectors.npz) and, for the production shape, against tests/cn_targets_contract.py,
which the CPU tests show equal to the fixture bit for bit.

Conditions per output: ind, reg_mask, wh and reg bit for bit; the support of hm and every cell equal to 1 exact, hm values within 1 fp32
ulp with at most 1 in 10^4 of the non-zero cells differing at all (the condition of tests/test_cp_targets_gpu.py: two float64
exponentials good to 1 ulp disagree after rounding to fp32 on about 2^-27 of the values).  Every output is pre-filled with garbage.
Then: from the original boxes plus matrix and flip through CenterNetTargets, equal results across calls, two streams and the
scratch-pool form, and the production shape."""
import functools

import numpy as np
import pytest
import torch

from tests import cn_targets_contract as ct
from tests.cp_loss_contract import ulps_apart
from tests.conftest import has_gpu
from tests.test_cn_targets_cpu import NAMES, fixture_case

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def garbage(B, kw):
    C, M, (W, H) = kw["num_classes"], kw["max_objs"], kw["feature_map_size"]
    out = dict(hm=torch.empty((B, C, H, W), device=DEV), ind=torch.empty((B, M), dtype=torch.int32, device=DEV),
               reg_mask=torch.empty((B, M), dtype=torch.uint8, device=DEV), wh=torch.empty((B, M, 2), device=DEV),
               reg=torch.empty((B, M, 2), device=DEV))
    for v in out.values():
        v.view(torch.uint8).fill_(0xFF)
    return out


def run(boxes, classes, kw, out=None):
    from minddet_amd import det_ops

    return det_ops.cn_assign_targets(dev(boxes), dev(classes), out=garbage(len(boxes), kw) if out is None else out, **kw)


def to_np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


def check(tag, got, want):
    """the conditions of the module docstring; prints the measured figures before it asserts"""
    for k in ct.KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
    nz = want["hm"] > 0
    apart = ulps_apart(got["hm"][nz], want["hm"][nz])
    ndiff, nnz = int((apart > 0).sum()), int(nz.sum())
    print(f"cn_targets[{tag}]: used slots {int(want['reg_mask'].sum())}, hm non-zero {nnz}, equal to 1 {int((want['hm'] == 1).sum())}, "
          f"differing {ndiff}, worst {int(apart.max())} ulp")
    for k in ("ind", "reg_mask", "wh", "reg"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert not np.isnan(got["hm"]).any() and np.array_equal(got["hm"] > 0, nz)            # support (and no garbage left)
    assert np.array_equal(got["hm"] == 1.0, want["hm"] == 1.0) and (want["hm"] == 1.0).sum() > 0
    assert int(apart.max()) <= 1 and ndiff * 10000 <= nnz, (int(apart.max()), ndiff, nnz)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_cases_equal_the_reference(name):
    inp, kw, want = fixture_case(name)
    check(name, to_np(run(inp["post_boxes"], inp["post_classes"], kw)), want)


@pytest.mark.parametrize("name", NAMES)
def test_from_original_boxes_through_the_targets_class(name):
    """CenterNetTargets: the flip, the affine transform and the truncation to max_objs on the device, then the operator"""
    from minddet_amd import det_ops

    inp, kw, want = fixture_case(name)
    tg = det_ops.CenterNetTargets(kw["num_classes"], kw["feature_map_size"], kw["max_objs"], kw["min_overlap"])
    out = tg(dev(inp["bboxes"]), dev(inp["category_id"]), dev(inp["trans_output"]), dev(inp["flip_width"]),
             out=garbage(len(inp["bboxes"]), kw))
    check(name + ", from the original boxes", to_np(out), want)


@functools.lru_cache(maxsize=None)
def production():
    """B = 16, 80 classes, 128 x 128, max_objs 128: G = 128 rows per image of which about 10 % are padding, boxes from 1 to 100 cells"""
    rng = np.random.default_rng(128)
    B, G = 16, 128
    c = rng.uniform(-4, 132, (B, G, 2))
    s = np.exp(rng.uniform(0, np.log(100.0), (B, G, 2)))
    boxes = np.concatenate([c - s / 2, c + s / 2], -1).astype(np.float32)
    classes = rng.integers(1, 81, (B, G)).astype(np.int32)
    pad = rng.uniform(size=(B, G)) < 0.1
    classes[pad] = np.where(rng.uniform(size=int(pad.sum())) < 0.5, 0, 81)
    kw = dict(num_classes=80, feature_map_size=(128, 128), max_objs=128, min_overlap=0.7)
    want = ct.assign(boxes, classes, **kw)
    for v in want.values():
        v.setflags(write=False)
    return boxes, classes, kw, want


def test_production_shape_equals_the_contract():
    boxes, classes, kw, want = production()
    assert want["reg_mask"].sum() > 1500 and (want["hm"].reshape(16 * 80, -1).max(1) == 0).any()   # empty planes among the 1280
    check("coco b16", to_np(run(boxes, classes, kw)), want)


def test_equal_across_calls_streams_and_the_scratch_pool():
    from minddet_amd import _lib
    from tests.abi_cases_cn import CNTargets

    inp, kw, want = fixture_case("small")
    boxes, classes = dev(inp["post_boxes"]), dev(inp["post_classes"])
    first = to_np(run(inp["post_boxes"], inp["post_classes"], kw))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs, pool = [garbage(2, kw), garbage(2, kw)], [garbage(2, kw), garbage(2, kw)]
    at = CNTargets()
    at.min_overlap = kw["min_overlap"]
    torch.cuda.synchronize()
    from minddet_amd import det_ops
    for rep in range(2):                                                          # the second round reuses each stream's pool buffer
        for s, o, q in zip(streams, outs, pool):
            with torch.cuda.stream(s):
                det_ops.cn_assign_targets(boxes, classes, out=o, **kw)
                assert _lib.call("md_cn_assign_targets", [boxes, classes, q["hm"], q["ind"], q["reg_mask"], q["wh"], q["reg"]], extra=at) == 0
    for o in [to_np(o) for o in outs + pool]:
        for k in ct.KEYS:
            assert np.array_equal(bits(first[k]), bits(o[k])), k                   # (a surviving 0xFF byte would differ from `first`)
    check("small, again", first, want)


def test_empty_rows_and_no_objects():
    """G = 0 and a batch of padding rows only: every output zero, every element written"""
    kw = dict(num_classes=3, feature_map_size=(70, 9), max_objs=5, min_overlap=0.7)
    for boxes, classes in ((np.zeros((2, 0, 4), np.float32), np.zeros((2, 0), np.int32)),
                           (np.full((2, 5, 4), 3.0, np.float32), np.zeros((2, 5), np.int32))):
        got = to_np(run(boxes, classes, kw))
        assert all(not v.view(np.uint8).any() for v in got.values())
