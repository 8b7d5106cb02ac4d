"""GPU: the CenterPoint training input (include/minddet_hip_cpaug.h) through the C ABI -- parity with the reference's own outputs
(tests/golden/cp_augment_vectors.npz) on every decided decision and with the float64 contract (tests/cpaug_contract.py) on the values,
a batch with an empty sample, straddling blocks, a sample without ground truth and one without candidates, a crowded select against
the contract's literal loop, a containment-only pair, determinism and the call forms, the chain into md_voxelize /
md_cp_assign_targets / the loss on the tiny config, the draws, and the ABI rows.

The rule for fp32 outputs is the one of tests/test_pc_augment_gpu.py: within 1 ulp of the contract's rounded value, at most 1 in 10^4
differing at all.  Integer and mask outputs are equal wherever the contract's decisions are decided; a count lies in
[decided-inside, decided-inside + undecided]."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import cpaug_contract as cc
from tests.conftest import has_gpu
from tests.cpaug_cases import NAMES, contract_case, fixture_case, has_candidates

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def to_np(t):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in t.items()}


def ulp32(got, want):
    """-> (largest distance in fp32 ulp, fraction of elements that differ at all)"""
    g, w = got.astype(np.float32).reshape(-1), want.astype(np.float32).reshape(-1)
    if g.size == 0:
        return 0.0, 0.0
    step = np.spacing(np.maximum(np.abs(w), np.float32(1e-30)).astype(np.float32)).astype(np.float64)
    return float((np.abs(g.astype(np.float64) - w.astype(np.float64)) / step).max()), float((g != w).mean())


def check32(what, got, want, few=1e-4):
    worst, frac = ulp32(got, want)
    print(f"{what}: worst {worst:.2f} ulp, differing {frac:.2e} of {got.size}")
    assert got.shape == want.shape and worst <= 1.0 and frac <= few, (what, worst, frac)


def run_ops(d, bv_range, min_points, workspace=True):
    """the four ops in the order of CenterPointAugment.__call__; d: device tensors (cand_* absent: no candidates)"""
    from minddet_amd import det_ops

    counts, keep = det_ops.cp_aug_count_points(d["points"], d["offsets"], d["gt_boxes"], d["gt_count"], min_points, workspace=workspace)
    if "cand_boxes" in d:
        accept = det_ops.cp_aug_select(d["gt_boxes"], d["gt_count"], keep, d["cand_boxes"], d["cand_count"], d["cand_group"], workspace=workspace)
        pts, offs = det_ops.cp_aug_points(d["points"], d["offsets"], d["glob"], d["cand_points"], d["cand_offsets"], d["cand_boxes"], accept,
                                          workspace=workspace)
        boxes, classes, count = det_ops.cp_aug_boxes(d["gt_boxes"], d["gt_classes"], d["gt_count"], keep, d["glob"], bv_range, d["cand_boxes"],
                                                     d["cand_classes"], accept)
    else:
        accept = None
        pts, offs = det_ops.cp_aug_points(d["points"], d["offsets"], d["glob"], workspace=workspace)
        boxes, classes, count = det_ops.cp_aug_boxes(d["gt_boxes"], d["gt_classes"], d["gt_count"], keep, d["glob"], bv_range)
    out = dict(counts=counts, keep=keep, points=pts, offsets=offs, gt_boxes=boxes, gt_classes=classes, gt_count=count)
    if accept is not None:
        out["accept"] = accept
    return out


def case_inputs(name):
    f = fixture_case(name)
    G, N = len(f["gt_boxes"]), len(f["points"])
    d = dict(points=dev(f["points"]), offsets=dev(np.array([0, N], np.int32)), gt_boxes=dev(f["gt_boxes"][None]), gt_classes=dev(f["gt_classes"][None]),
             gt_count=dev(np.array([G], np.int32)), glob=dev(f["global"][None]))
    if has_candidates(f):
        S = len(f["cand_boxes"])
        d.update(cand_boxes=dev(f["cand_boxes"][None]), cand_classes=dev(f["cand_classes"][None]), cand_group=dev(f["cand_group"][None]),
                 cand_count=dev(np.array([S], np.int32)), cand_points=dev(f["cand_points"]), cand_offsets=dev(f["cand_offsets"]))
    return d


@functools.lru_cache(maxsize=None)
def device_case(name):
    f = fixture_case(name)
    out = to_np(run_ops(case_inputs(name), f["bv_range"], int(f["min_points"])))
    torch.cuda.synchronize()
    return out


def check_against_contract(tag, got, c):
    """one sample of the device's result (counts [G], keep [G], accept [S] or absent, points [rows, 5] = the sample's slice of
    points_out, gt_boxes [G+S, 9], gt_classes, gt_count) against the contract's (see contract_case) -> every decision was decided"""
    cnt = c["count"]
    assert ((got["counts"] >= cnt["lo"]) & (got["counts"] <= cnt["hi"])).all(), (tag, got["counts"].tolist(), cnt["lo"].tolist(), cnt["hi"].tolist())
    same = cnt["lo"] == cnt["hi"]
    assert np.array_equal(got["counts"][same], cnt["counts"][same]), tag
    kd = cnt["keep_decided"]
    assert np.array_equal(got["keep"][kd], cnt["keep"][kd]), tag
    if not np.array_equal(got["keep"], cnt["keep"]):
        return False                                       # an undecided keep: what follows was computed from another mask
    if c["accept"] is not None:
        assert np.array_equal(got["accept"], c["accept"]), (tag, got["accept"].tolist(), c["accept"].tolist())
    p = c["pts"]
    assert len(got["points"]) == len(p["points"]), tag
    check32(tag + " points", got["points"][:, :3], p["points"][:, :3])
    assert np.array_equal(got["points"][:, 3:].view(np.uint32), p["points"][:, 3:].view(np.uint32)), tag
    b = c["boxes"]
    dec = b["margin"] > cc.MARGIN
    n = int(got["gt_count"])
    assert int((b["mask"] & dec).sum()) <= n <= int((b["mask"] & dec).sum() + (~dec).sum()), tag
    assert not got["gt_boxes"][n:].any() and not got["gt_classes"][n:].any(), tag
    if dec.all():
        assert n == b["count"] and np.array_equal(got["gt_classes"], b["gt_classes"]), tag
        check32(tag + " gt_boxes", got["gt_boxes"], b["gt_boxes"])
    else:
        # the decided survivors are there, in order, with the contract's values; an undecided row may sit between them
        want = b["all"][b["mask"] & dec].astype(np.float32)
        at = 0
        for row in want:
            while at < n and not (np.abs(got["gt_boxes"][at].astype(np.float64) - row) <= 2 * np.spacing(np.abs(row)) + 1e-30).all():
                at += 1
            assert at < n, (tag, "a decided survivor is missing")
            at += 1
    return bool(cnt["decided"] and dec.all())


@pytest.mark.parametrize("name", NAMES)
def test_parity_with_the_reference_and_the_contract(name):
    f, c, got = fixture_case(name), contract_case(name), device_case(name)
    one = {k: (v[0] if k in ("counts", "keep", "accept", "gt_boxes", "gt_classes", "gt_count") else v) for k, v in got.items()}
    # the reference's own decisions
    cnt = c["count"]
    same = cnt["lo"] == cnt["hi"]
    assert np.array_equal(one["counts"][same], f["counts"][same]) and np.array_equal(one["keep"], f["keep"])
    if has_candidates(f):
        assert np.array_equal(one["accept"], f["accept"])
    k = len(f["points_translate"])
    assert one["offsets"].tolist() == [0, k] and not one["points"][k:].any()
    assert np.array_equal(one["points"][:k, 3:].view(np.uint32), f["points_translate"][:, 3:].view(np.uint32))
    dec = c["boxes"]["margin"] > cc.MARGIN
    if dec.all():
        assert int(one["gt_count"]) == len(f["final_boxes"]) and np.array_equal(one["gt_classes"][:len(f["final_boxes"])], f["final_classes"])
    one["points"] = one["points"][:k]
    decided = check_against_contract(name, one, c)
    assert decided == (name != "plants")                   # nothing is left out silently
    if name == "plants":
        face = one["counts"][0] - 3                        # three points well inside, nine on the faces
        assert 0 <= face <= 9 and 3 <= int(one["gt_count"]) <= 5      # rows 0, 1, 3 decided in, rows 2 and 4 on the edge
    if name == "order":
        assert one["accept"].tolist() == [0, 1, 0, 0, 1, 1, 1, 0, 0, 1, 1]


def split_candidates(s, b):
    """sample b's candidate operands of a batch dict as the contract takes them"""
    S = s["cand_boxes"].shape[1]
    offs = s["cand_offsets"][b * S:(b + 1) * S + 1]
    return s["cand_points"], offs


def contract_batch(s, b, min_points, bv):
    G = s["gt_boxes"].shape[1]
    n0, n1 = s["offsets"][b], s["offsets"][b + 1]
    pts = s["points"][n0:n1]
    gc = int(s["gt_count"][b])
    cnt = cc.count_points(pts, s["gt_boxes"][b], gc, min_points)
    if "cand_boxes" in s:
        cpts, coffs = split_candidates(s, b)
        accept = cc.select(s["gt_boxes"][b], gc, cnt["keep"], s["cand_boxes"][b], int(s["cand_count"][b]), s["cand_group"][b])
        p = cc.augment_points(pts, s["glob"][b], cpts, coffs, s["cand_boxes"][b], accept)
        bx = cc.augment_boxes(s["gt_boxes"][b], s["gt_classes"][b], gc, cnt["keep"], s["glob"][b], bv, s["cand_boxes"][b], s["cand_classes"][b], accept)
    else:
        accept = None
        p = cc.augment_points(pts, s["glob"][b])
        bx = cc.augment_boxes(s["gt_boxes"][b], s["gt_classes"][b], gc, cnt["keep"], s["glob"][b], bv)
    assert G == len(cnt["keep"])
    return dict(count=cnt, accept=accept, pts=p, boxes=bx)


def batch3(sizes=(0, 300, 2050)):
    """B = 3: an empty sample without ground truth, 300 and 2 050 points (blocks that straddle samples, several blocks per sample);
    G = 6, S = 5; the last sample has no candidates (cand_count 0) though its rows are filled"""
    rng = np.random.default_rng(5)
    G, S = 6, 5
    boxes = np.zeros((3, G, 9), np.float32)
    for b in range(3):
        for g in range(G):
            boxes[b, g] = (-40 + 15 * g + rng.uniform(-1, 1), rng.uniform(-30, 30), -1.0, 1.9, 4.5, 1.7, rng.uniform(-3, 3), rng.uniform(-3, 3),
                           rng.uniform(-3, 3))
    gt_count = np.array([0, 6, 5], np.int32)
    pts = []
    for b, n in enumerate(sizes):
        inside = boxes[b, rng.integers(0, G, n), :3] + rng.uniform(-1.2, 1.2, (n, 3))
        bg = np.stack([rng.uniform(-51, 51, n), rng.uniform(-51, 51, n), rng.uniform(-2.5, 0.5, n)], 1)
        xyz = np.where((rng.uniform(size=n) < 0.5)[:, None], inside, bg)
        pts.append(np.concatenate([xyz, rng.uniform(0, 1, (n, 2))], 1).astype(np.float32))
    for b in range(3):                                     # no point within the margin of a face: every count is decided
        near = (np.abs(cc.signed_inside(pts[b], boxes[b])) <= 4 * cc.MARGIN).any(1) if len(pts[b]) else np.zeros(0, bool)
        pts[b][near, 2] = 5.0
    cand = np.zeros((3, S, 9), np.float32)
    for b in range(3):
        for k in range(S):
            on_top = boxes[b, k] if k % 2 == 0 else None
            cand[b, k] = (rng.uniform(-45, 45), rng.uniform(-45, 45), -1.0, 2.0, 4.6, 1.7, rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-3, 3))
            if on_top is not None and k < 4:
                cand[b, k, :2] = on_top[:2] + 0.5
    per = rng.integers(3, 30, (3, S))
    cand_points = np.concatenate([rng.uniform(-1, 1, (int(per.sum()), 3)), rng.uniform(0, 1, (int(per.sum()), 2))], 1).astype(np.float32)
    cand_offsets = np.concatenate([[0], np.cumsum(per.reshape(-1))]).astype(np.int32)
    glob = np.array([[1, 0, 0.3, 1.02, 0.1, -0.2, 0.05], [0, 1, -0.35, 0.97, -0.3, 0.1, 0.0], [1, 1, 0.2, 1.04, 0.2, 0.2, -0.1]], np.float64)
    return dict(points=np.concatenate(pts), offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), gt_boxes=boxes, gt_count=gt_count,
                gt_classes=np.array([[1, 2, 0, 3, 1, 2]] * 3, np.int32), cand_boxes=cand, cand_classes=np.array([[1, 1, 2, 0, 3]] * 3, np.int32),
                cand_group=np.array([[0, 0, 0, 1, 1], [2, 2, 5, 5, 7], [0, 1, 2, 3, 4]], np.int32), cand_count=np.array([5, 5, 0], np.int32),
                cand_points=cand_points, cand_offsets=cand_offsets, glob=glob)


def batch_dev(s):
    return {k: dev(v) for k, v in s.items()}


def check_batch(tag, s, got, min_points, bv):
    B = len(s["gt_count"])
    offs = got["offsets"]
    assert offs[0] == 0 and (np.diff(offs) >= 0).all() and not got["points"][offs[B]:].any()
    decided = []
    for b in range(B):
        c = contract_batch(s, b, min_points, bv)
        one = dict(counts=got["counts"][b], keep=got["keep"][b], points=got["points"][offs[b]:offs[b + 1]], gt_boxes=got["gt_boxes"][b],
                   gt_classes=got["gt_classes"][b], gt_count=got["gt_count"][b])
        if "accept" in got:
            one["accept"] = got["accept"][b]
        decided.append(check_against_contract(f"{tag} sample {b}", one, c))
    return decided


def test_batch_with_an_empty_sample_and_straddling_blocks():
    s = batch3()
    bv = (-51.2, -51.2, 51.2, 51.2)
    got = to_np(run_ops(batch_dev(s), bv, 10))
    decided = check_batch("batch3", s, got, 10, bv)
    assert all(decided)
    assert got["offsets"][1] == 0 + int(np.diff(s["cand_offsets"][:6])[got["accept"][0] != 0].sum())      # the empty sample: its candidates' points only
    assert not got["counts"][0].any() and not got["keep"][0].any() and got["accept"][0].any()
    assert not got["accept"][2].any() and got["offsets"][3] - got["offsets"][2] == 2050
    assert 0 < got["accept"][1].sum() < 5 and (got["keep"][1] == 0).any() and got["keep"][1].any()
    assert len(got["points"]) == 2350 + len(s["cand_points"]) and got["offsets"][3] < len(got["points"])


def test_compaction_with_more_block_counts_than_one_scan_pass():
    """256 * 256 + 1 scene points and the candidates' in front of them: more than 256 block counts, so the one-workgroup scan of the
    counts takes a second pass and carries the first's total"""
    s = batch3(sizes=(0, 300, 256 * 256 + 1 - 300))
    bv = (-51.2, -51.2, 51.2, 51.2)
    got = to_np(run_ops(batch_dev(s), bv, 10))
    assert all(check_batch("batch3 x 257 blocks", s, got, 10, bv))
    assert len(got["points"]) > 256 * 256 and got["offsets"][3] > 256 * 256 and got["points"][got["offsets"][3] - 1].any()


def crowded():
    rng = np.random.default_rng(21)
    B, G, S = 3, 40, 70
    def boxes(n):
        b = np.zeros((B, n, 9), np.float32)
        b[..., 0], b[..., 1], b[..., 2] = rng.uniform(-10, 10, (B, n)), rng.uniform(-10, 10, (B, n)), -1.0
        b[..., 3], b[..., 4], b[..., 5] = rng.uniform(0.6, 2.2, (B, n)), rng.uniform(0.8, 5.0, (B, n)), 1.6
        b[..., 8] = rng.uniform(-3, 3, (B, n))
        return b
    keep = (rng.uniform(size=(B, G)) < 0.4).astype(np.uint8)
    group = np.sort(rng.integers(0, 4, (B, S)), axis=1).astype(np.int32)
    return dict(gt=boxes(G), keep=keep, gt_count=np.array([40, 33, 40], np.int32), cand=boxes(S), cand_count=np.array([70, 55, 70], np.int32), group=group)


def test_crowded_select_equals_the_contracts_literal_loop():
    """G + S = 110 columns: rows and columns cross the 64-bit word and the wave boundary; most candidates are rejected, some are
    accepted in later groups, some only because what they collide with was rejected or dropped"""
    from minddet_amd import det_ops

    s = crowded()
    for workspace in (True, False):
        later = high = 0
        acc = det_ops.cp_aug_select(dev(s["gt"]), dev(s["gt_count"]), dev(s["keep"]), dev(s["cand"]), dev(s["cand_count"]), dev(s["group"]),
                                    workspace=workspace).cpu().numpy()
        for b in range(3):
            want = cc.select(s["gt"][b], int(s["gt_count"][b]), s["keep"][b], s["cand"][b], int(s["cand_count"][b]), s["group"][b])
            assert np.array_equal(acc[b], want), (b, acc[b].tolist(), want.tolist())
            n = int(s["cand_count"][b])
            print(f"crowded sample {b}: accepted {int(want.sum())} of {n}, by group {[int(want[:n][s['group'][b, :n] == g].sum()) for g in range(4)]}")
            assert want.sum() < n / 2 and want[:n][s["group"][b, :n] >= 1].any()
            later += int(want[:n][s["group"][b, :n] >= 2].sum())
            high += int(want[64:n].sum())
        assert not acc[1, 55:].any() and acc.sum() >= 12 and later >= 3 and high >= 1      # accepted in the last groups, and in the row's second word
    # a group sequence that decreases: that sample accepts nothing, the others are not touched
    bad = s["group"].copy()
    bad[1, 10] = 3
    acc2 = det_ops.cp_aug_select(dev(s["gt"]), dev(s["gt_count"]), dev(s["keep"]), dev(s["cand"]), dev(s["cand_count"]), dev(bad)).cpu().numpy()
    assert not acc2[1].any() and np.array_equal(acc2[0], acc[0]) and np.array_equal(acc2[2], acc[2])


def test_containment_only_pairs_collide():
    """quirk (a): a box wholly inside another has no crossing edges; the predicate's containment tests reject it (the fixture's
    generator cannot pin this: under its shim the reference skips them)"""
    from minddet_amd import det_ops

    gt = np.array([[[0, 0, -1, 8.0, 9.0, 2, 0, 0, 0.3], [30, 0, -1, 0.6, 0.8, 1.7, 0, 0, -1.0]]], np.float32)
    cand = np.array([[[0.2, -0.1, -1, 0.6, 0.8, 1.7, 0, 0, 1.1],           # inside ground-truth row 0
                      [30.1, 0.1, -1, 8.0, 9.0, 2, 0, 0, 0.7],              # around ground-truth row 1
                      [-30, 20, -1, 2.0, 4.0, 1.7, 0, 0, 0.2],              # free
                      [-30.1, 20.2, -1, 0.5, 0.5, 1.7, 0, 0, 2.0]]], np.float32)      # inside the accepted candidate of the group before
    group = np.array([[0, 0, 0, 1]], np.int32)
    args = (gt[0], 2, np.ones(2, np.uint8), cand[0], 4, group[0])
    x, y = cc.bev_corners(np.concatenate([gt[0], cand[0]]))
    edges, a_b, b_a, hit = cc.collide(x[:, None], y[:, None], x[None], y[None])
    assert hit[2, 0] and not edges[2, 0] and hit[3, 1] and not edges[3, 1] and hit[5, 4] and not edges[5, 4]
    want = cc.select(*args)
    assert want.tolist() == [0, 0, 1, 0]
    acc = det_ops.cp_aug_select(dev(gt), dev(np.array([2], np.int32)), dev(np.ones((1, 2), np.uint8)), dev(cand), dev(np.array([4], np.int32)), dev(group))
    assert acc.cpu().numpy()[0].tolist() == want.tolist()


def test_determinism_and_call_forms():
    s = batch3()
    d, bv = batch_dev(s), (-51.2, -51.2, 51.2, 51.2)
    first = run_ops(d, bv, 3)
    again = run_ops(d, bv, 3)
    pool = run_ops(d, bv, 3, workspace=False)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = run_ops(d, bv, 3)
    torch.cuda.synchronize()
    for k, v in first.items():
        raw = v.view(torch.uint8)
        for tag, o in (("again", again), ("pool", pool), ("second stream", other)):
            assert torch.equal(raw, o[k].view(torch.uint8)), (k, tag)
    want = device_case("nusc")
    got = to_np(run_ops(case_inputs("nusc"), fixture_case("nusc")["bv_range"], 5, workspace=False))
    assert all(np.array_equal(got[k], want[k]) for k in want)


def _model():
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_tiny_points_train.py"))
    return build_detector(dict(cfg.model), dict(cfg.train_cfg), cfg.test_cfg).to(DEV), cfg


def test_chain_into_voxeliser_targets_and_loss():
    from minddet_amd import det_ops

    m, cfg = _model()
    rng = np.random.default_rng(8)
    B, G, S, n = 3, 6, 3, 1500
    boxes = np.zeros((B, G, 9), np.float32)
    for b in range(B):
        for g in range(G):
            boxes[b, g] = (-5 + 2 * g + rng.uniform(-0.2, 0.2), rng.uniform(-3.5, 3.5), -1.0, 0.8, 1.6, 1.5, rng.uniform(-2, 2), rng.uniform(-2, 2),
                           rng.uniform(-3, 3))
    count = np.array([6, 1, 4], np.int32)
    classes = np.tile(np.array([[1, 2, 3, 0, 1, 2]], np.int32), (B, 1))
    pts = []
    for b in range(B):
        inside = boxes[b, rng.integers(0, G, n), :3] + rng.uniform(-0.3, 0.3, (n, 3))
        bg = np.stack([rng.uniform(-6.4, 6.4, n), rng.uniform(-6.4, 6.4, n), rng.uniform(-3, 1, n)], 1)
        xyz = np.where((rng.uniform(size=n) < 0.3)[:, None], inside, bg)
        pts.append(np.concatenate([xyz, rng.uniform(0, 1, (n, 2))], 1).astype(np.float32))
    offs = np.arange(B + 1, dtype=np.int32) * n
    cand = np.zeros((B, S, 9), np.float32)
    cand[:, 0] = (4.0, 5.5, -1.0, 0.8, 1.6, 1.5, 1.0, 0.5, 0.4)
    cand[:, 1] = boxes[:, 0] + np.array([0.1, 0.1, 0, 0, 0, 0, 0, 0, 0.5], np.float32)      # on ground-truth row 0: rejected where that row is kept
    cand[:, 2] = (-4.0, -5.6, -1.0, 0.6, 0.6, 1.7, 0.0, 0.0, -1.0)
    per = np.full((B, S), 40)
    cand_points = np.concatenate([rng.uniform(-0.3, 0.3, (B * S * 40, 3)), rng.uniform(0, 1, (B * S * 40, 2))], 1).astype(np.float32)
    sampled = dict(points=dev(cand_points), offsets=dev(np.concatenate([[0], np.cumsum(per.reshape(-1))]).astype(np.int32)), boxes=dev(cand),
                   classes=dev(np.array([[1, 2, 3]] * B, np.int32)), group=dev(np.array([[0, 0, 1]] * B, np.int32)), count=dev(np.array([3, 3, 2], np.int32)))
    args = (dev(np.concatenate(pts)), dev(offs), dev(boxes), dev(classes), dev(count))
    aug = m.augment_op()
    assert aug.min_points_in_gt == 2 and aug.global_translate_std == (0.2, 0.2, 0.2) and m.targets_op().max_objs == 32
    draws = aug.draw(B, torch.Generator(device=DEV).manual_seed(3))
    ex = m.train_example(*args, draws=draws, sampled=sampled)
    a = ex["augment"]
    p_np, o_np, acc = a["points"].cpu().numpy(), a["offsets"].cpu().numpy(), a["accept"].cpu().numpy()
    assert acc[:, 0].all() and not acc[:, 1].any() and acc[:2, 2].all() and not acc[2, 2]      # (sample 2 draws two candidates)
    kept = n + 40 * acc.sum(1)
    assert o_np.tolist() == [0] + np.cumsum(kept).tolist() and o_np[-1] < len(p_np) and not p_np[o_np[-1]:].any()
    # md_voxelize on the op's output (zero rows behind the last kept one) == md_voxelize on the kept rows alone
    host = np.ascontiguousarray(p_np[:o_np[-1]])
    mv = cfg.train_cfg["max_voxel_num"]
    vox_a = det_ops.voxelize(a["points"], a["offsets"], m.voxel_size, m.pc_range, m.max_points, mv)
    vox_b = det_ops.voxelize(dev(host), dev(o_np), m.voxel_size, m.pc_range, m.max_points, mv)
    for x, y in zip(vox_a, vox_b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # the targets of the fixed-capacity list (padding rows: class 0) == the targets of each sample's host-sliced list
    n_out = a["gt_count"].cpu().numpy()
    assert (n_out >= 1).all() and n_out[0] >= 3 and a["gt_boxes"].shape == (B, G + S, 9)
    tg = m.targets_op()
    for b in range(B):
        k = int(n_out[b])
        want = tg(a["gt_boxes"][b:b + 1, :k].contiguous(), a["gt_classes"][b:b + 1, :k].contiguous())
        for key, w in want.items():
            assert torch.equal(ex[key][b:b + 1].contiguous().view(torch.uint8), w.view(torch.uint8)), (b, key)
    one = m.train_loss(*args, draws=draws, sampled=sampled, grad=True)
    two = m.train_loss(*args, draws=draws, sampled=sampled, grad=True)
    torch.cuda.synchronize()
    for k in ("total", "parts", "num_pos", "grad"):
        assert torch.isfinite(one[k].float()).all() and torch.equal(one[k].view(torch.uint8), two[k].view(torch.uint8)), k
    assert torch.equal(one["example"]["hm"], ex["hm"]) and float(one["total"]) > 0
    g1 = m.train_loss(*args, generator=torch.Generator(device=DEV).manual_seed(3), sampled=sampled)      # the same generator state: the same draws
    assert torch.equal(g1["total"], one["total"])
    plain = m.train_loss(*args, draws=draws)               # without the sampler
    assert plain["example"]["augment"]["accept"] is None and torch.isfinite(plain["total"]).all()
    assert plain["example"]["augment"]["gt_boxes"].shape == (B, G, 9)


def test_draw_follows_the_reference_distributions():
    from minddet_amd import det_ops

    aug = det_ops.CenterPointAugment((-51.2, -51.2, 51.2, 51.2), [-0.3925, 0.3925], [0.95, 1.05], global_translate_std=[0.2, 0.5, 9.0])
    g = aug.draw(4096, torch.Generator(device=DEV).manual_seed(1)).cpu().numpy()
    assert g.shape == (4096, 7) and g.dtype == np.float64
    for k in (0, 1):                                       # Bernoulli(0.5): the standard error of the mean is 0.0078
        assert set(np.unique(g[:, k]).tolist()) == {0.0, 1.0} and abs(g[:, k].mean() - 0.5) <= 0.05
    assert abs((g[:, 0] * g[:, 1]).mean() - 0.25) <= 0.05                     # independent
    assert (np.abs(g[:, 2]) <= 0.3925).all() and np.ptp(g[:, 2]) > 0.77 and abs(g[:, 2].mean()) <= 0.03
    assert (g[:, 3] >= 0.95).all() and (g[:, 3] <= 1.05).all() and np.ptp(g[:, 3]) > 0.098
    for k, std in ((4, 0.2), (5, 0.5), (6, 0.2)):         # z is drawn with std[0]; 4 096 draws: the standard error of the std is 1.1 %
        assert abs(g[:, k].std() / std - 1.0) <= 0.10, (k, g[:, k].std())
    still = det_ops.CenterPointAugment((-51.2, -51.2, 51.2, 51.2), 0.3925, [0.95, 1.05])
    z = still.draw(8, torch.Generator(device=DEV).manual_seed(2))
    assert not z[:, 4:].any() and torch.equal(z, still.draw(8, torch.Generator(device=DEV).manual_seed(2)))
