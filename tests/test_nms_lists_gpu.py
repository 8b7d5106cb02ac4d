"""-m gpu: the NMS kernels of csrc/nms.hip on clustered, chained, lattice and ragged lists, judged by the float64 contract of
tests/nms_contract.py (validity of the keep list under derived error bands; equality in the lattice regime), through the C ABI as
det_ops calls it.  Every output lives between sentinel guards, every case runs twice and the two runs agree byte for byte.  The
shapes are the smallest that reach each path of nms_scan_kernel and of the quota prefix pass, not the workloads' own;
tests/test_nms_contract_cpu.py pins the same lists and the contract itself without a GPU."""
import numpy as np
import pytest
import torch

from tests import nms_contract as nc
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]

DEV = "cuda:0"
GUARD = 1 << 12
FILL = {torch.uint8: 0xA5, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.float32: -12345.0}
ALIGNED_OP = {0: "ge", 1: "gt", 2: "gt"}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(shape, dtype):
    """(tensor, flat): an output of `shape` filled with a sentinel inside a sentinel buffer GUARD elements longer on each side"""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), FILL[dtype], dtype=dtype, device=DEV)
    return flat[GUARD:GUARD + n].view(shape), flat


def call_twice(sym, inputs, out_specs, extra=None, workspace=None):
    """Run the op twice into fresh guarded outputs: guards intact, both runs byte-equal; returns the outputs as numpy arrays."""
    from minddet_amd import _lib

    runs = []
    for _ in range(2):
        outs = [guarded(shape, dtype) for shape, dtype in out_specs]
        params = list(inputs) + [o for o, _ in outs]
        if workspace is not None:
            params.append(workspace)
        _lib.call(sym, params, extra=extra)
        torch.cuda.synchronize()
        for (o, flat), (shape, dtype) in zip(outs, out_specs):
            assert bool((flat[:GUARD] == FILL[dtype]).all()) and bool((flat[-GUARD:] == FILL[dtype]).all()), f"{sym}: write outside an output"
        runs.append([flat for _, flat in outs])
    for a, b in zip(*runs):
        assert torch.equal(a, b), f"{sym}: two runs of one call differ"
    return [flat[GUARD:-GUARD].view(shape).cpu().numpy() for flat, (shape, _) in zip(runs[0], out_specs)]


def aligned_workspace(B, n, mask_only=False):
    """(workspace, mask bytes): det_ops.nms_aligned's workspace for md_nms_aligned, the suppression mask and one flag per list
    behind it, or the mask alone; filled with 0xA5 so that what the op writes behind the mask can be told."""
    mask_bytes = B * n * ((n + 63) // 64) * 8
    return torch.full((mask_bytes + (0 if mask_only else (B * 4 + 255) // 256 * 256),), 0xA5, dtype=torch.uint8, device=DEV), mask_bytes


def run_aligned(boxes, count, group, thr, mode, quota=0, ws=None):
    """md_nms_aligned on boxes[B,n,4] -> (keep_mask[B,n], keep_idx[B,n], num[B]); ws: aligned_workspace(B, n) unless given."""
    from minddet_amd import det_ops

    B, n = boxes.shape[:2]
    ws = aligned_workspace(B, n)[0] if ws is None else ws
    inputs = [T(boxes.astype(np.float32)), None if count is None else T(count.astype(np.int32)), None if group is None else T(group.astype(np.int32))]
    return call_twice("md_nms_aligned", inputs, [((B, n), torch.uint8), ((B, n), torch.int32), ((B,), torch.int32)],
                      extra=det_ops._NmsAttrs(float(thr), 0.0, int(mode), int(quota)), workspace=ws)


def judge_aligned(boxes, m, group, outs, l, mode, thr, quota=0, exact=False):
    mask, idx, num = outs
    n = boxes.shape[0]
    keep = nc.keep_from_outputs(n, num[l], idx[l], mask[l])
    band = nc.aligned_band(boxes, mode, exact=exact)
    und, jud = nc.judge_greedy(band, m, keep, groups=group, quota=quota, op=ALIGNED_OP[mode], thr=thr)
    if exact:
        assert und == 0
        np.testing.assert_array_equal(keep, nc.greedy_exact(band, m, groups=group, quota=quota, op=ALIGNED_OP[mode], thr=thr))
    return keep


def run_keep_list(sym, boxes, thr, dtype):
    keep, num = call_twice(sym, [T(np.asarray(boxes, np.float32)), T(np.array([thr], np.float32))], [((len(boxes),), dtype), ((1,), torch.int32)])
    return nc.keep_from_outputs(len(boxes), num[0], keep)


def run_circle(xy, thr):
    mask, idx, num = call_twice("md_circle_nms", [T(np.asarray(xy, np.float32)), T(np.array([thr], np.float32))],
                                [((len(xy),), torch.uint8), ((len(xy),), torch.int32), ((1,), torch.int32)])
    return nc.keep_from_outputs(len(xy), num[0], idx, mask)


# ------------------------------------------------------------------------------------------------ md_nms_aligned
@pytest.mark.parametrize("n", nc.ALIGNED_NS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_aligned_batches_pass_the_judge(mode, n):
    """B = 6 lists in one launch (class keys 5 / 80 / 1, chain, lattice, NaN and inf boxes), count in {0, 1, 64, n-5, n, n+7}."""
    for thr in nc.ALIGNED_THRS:
        boxes, count, group, kinds = nc.aligned_batch(n, mode, thr, 100 * n + mode)
        outs = run_aligned(boxes, count, group, thr, mode)
        for l, kind in enumerate(kinds):
            m = min(int(count[l]), n)                      # the count clamp
            keep = judge_aligned(boxes[l], m, group[l], outs, l, mode, thr, exact=kind == "lattice" and n >= 63)
            assert m == 0 or keep[0] == 0


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_aligned_full_lists(mode):
    """640-box chain (the odd boxes survive: a suppressed box suppresses nothing, across ten tile boundaries), lattice list (the one
    exact keep list), NaN / inf list (both kept: NaN compares false) and an 80-class clustered list, in one launch."""
    for thr in nc.ALIGNED_THRS:
        boxes, group, kinds = nc.aligned_full_lists(mode, thr, 40 + mode)
        outs = run_aligned(boxes, None, group, thr, mode)
        for l, kind in enumerate(kinds):
            keep = judge_aligned(boxes[l], 640, group[l], outs, l, mode, thr, exact=kind == "lattice")
            if kind == "chain":
                np.testing.assert_array_equal(keep, np.concatenate([[0], np.arange(1, 640, 2)]))
            if kind == "naninf":      # the all-NaN box in every mode; partly NaN and infinite boxes where the quotient is unclamped
                assert 640 // 3 in keep
                if mode != 2:
                    assert np.isin([640 // 4, 2 * 640 // 3, 640 // 5, 3 * 640 // 4, 640 // 2], keep).all()


@pytest.mark.parametrize("thr", [0.5, 0.25])
def test_aligned_lattice_ties(thr):
    """IoU exactly thr: mode 0 (>=) suppresses, modes 1 and 2 (>) keep; modes 0 and 2 differ on exactly the four planted pairs."""
    keeps = {}
    for mode in (0, 1, 2):
        b = nc.lattice_ties(mode, thr)
        outs = run_aligned(b[None], None, None, thr, mode)
        keeps[mode] = judge_aligned(b, len(b), None, outs, 0, mode, thr, exact=True)
        second = np.arange(1, len(b), 6)
        assert np.isin(second, keeps[mode]).all() == (mode != 0) and np.isin(second, keeps[mode]).any() == (mode != 0)
        assert not np.isin(second + 2, keeps[mode]).any() and np.isin(second + 4, keeps[mode]).all()
    assert len(keeps[2]) - len(keeps[0]) == 4


def test_aligned_zero_area_rows():
    """No dead-area rule in md_nms_aligned: four all-zero rows are all kept in modes 0 (0/0 = NaN) and 2 (0 / 1e-8 = 0); mode 1
    gives each an area of one pixel, ovr 1, and keeps the first."""
    z = np.zeros((1, 4, 4), np.float32)
    for mode, want in nc.ZERO_ROWS_KEPT.items():
        mask, idx, num = run_aligned(z, None, None, 0.5, mode)
        assert nc.keep_from_outputs(4, num[0], idx[0], mask[0]).tolist() == want


@pytest.mark.parametrize("quota", [1, 63, 64, 65])
def test_aligned_quota_ends_inside_a_block(quota):
    """max_output in {1, 63, 64, 65} on 640-box lists, among them one whose survivors number exactly the quota and one that is a
    single survivor short."""
    rng = np.random.default_rng(quota)
    full = np.concatenate([np.arange(quota), rng.integers(0, quota, 640 - quota)])
    short = np.concatenate([np.arange(quota - 1), rng.integers(0, max(quota - 1, 1), 640 - quota + 1)])[:640]
    for mode in (0, 1, 2):
        boxes, _, group, _ = nc.aligned_batch(640, mode, 0.5, 900 + quota)
        boxes = np.concatenate([boxes[:4], np.stack([nc.slot_aligned(p, quota + i) for i, p in enumerate((full, short))])])
        group = np.concatenate([group[:4], np.zeros((2, 640), np.int32)])
        outs = run_aligned(boxes, None, group, 0.5, mode, quota=quota)
        keeps = [judge_aligned(boxes[l], 640, group[l], outs, l, mode, 0.5, quota=quota) for l in range(6)]
        assert len(keeps[4]) == quota and keeps[4][-1] == quota - 1 and len(keeps[5]) == (quota - 1 if quota > 1 else 1)


@pytest.mark.parametrize("quota,n", [(100, 1023), (100, 1024), (100, 1100), (300, 2431), (300, 2432), (300, 2500)])
def test_quota_prefix_pass(quota, n):
    """The two production quotas around the length 2 P at which md_nms_aligned starts with a prefix pass: in one batch a list that
    fills the quota at box P-1, one that needs box P, one whose prefix collapses (the gated full pass runs), lists shorter than P
    and an empty one.  All judged; and byte-equal to the single full pass a mask-only workspace gives."""
    boxes, count, group, P = nc.quota_prefix_batch(n, quota, quota + n)
    ws, mask_bytes = aligned_workspace(6, n)
    outs = run_aligned(boxes, count, group, 0.5, 2, quota=quota, ws=ws)
    flags = ws[mask_bytes:mask_bytes + 24].view(torch.int32).cpu().tolist()
    keeps = [judge_aligned(boxes[l], min(int(count[l]), n), group[l], outs, l, 2, 0.5, quota=quota) for l in range(6)]
    assert len(keeps[0]) == quota and keeps[0][-1] == P - 1
    assert len(keeps[1]) == quota and keeps[1][-1] == P
    assert (keeps[2] < P).sum() == 3 and len(keeps[2]) == min(quota, 3 + max(n - P - 90, 0))
    assert len(keeps[5]) == 0
    single = run_aligned(boxes, count, group, 0.5, 2, quota=quota, ws=aligned_workspace(6, n, mask_only=True)[0])
    for a, b in zip(outs, single):
        np.testing.assert_array_equal(a, b)
    # which path ran is visible in the workspace: the prefix pass leaves one flag per list behind the mask (1 = the full pass has to
    # redo this list); below 2 P boxes, and with a workspace of another size than the op asks for, nothing is written there
    if n >= 2 * P:
        assert flags == [int(count[l] > P and (keeps[l] < P).sum() < quota) for l in range(6)] and sum(flags) >= 2
    else:
        assert all(f == int.from_bytes(b"\xa5" * 4, "little", signed=True) for f in flags)
    # and the production wrapper, with the workspace it allocates itself, gives the same bytes
    from minddet_amd import det_ops
    m2, i2, n2 = det_ops.nms_aligned(T(boxes), 0.5, mode=2, count=T(count), group=T(group), max_output=quota)
    for a, b in zip(outs, (m2, i2, n2)):
        np.testing.assert_array_equal(a, b.cpu().numpy())


def test_kept_rows_past_the_scan_cap():
    """4288 disjoint lattice boxes, all kept, then exact copies of the kept boxes of rank 4100..4227: their suppressors' row indices
    are past the SCAN_KEEP_CAP entries nms_scan_kernel holds in LDS and are read back from its keep output (int32 and int64)."""
    b4, xy, b7 = nc.rank_cap_lists()
    want = np.arange(4288)
    mask, idx, num = run_aligned(b4[None], None, None, 0.5, 2)
    np.testing.assert_array_equal(nc.keep_from_outputs(len(b4), num[0], idx[0], mask[0]), want)
    np.testing.assert_array_equal(run_circle(xy, 4.0), want)
    np.testing.assert_array_equal(run_keep_list("NmsNormalGpu", b7, 0.5, torch.int64), want)


# ------------------------------------------------------------------------------------------------ NmsNormalGpu, md_circle_nms
def test_normal_lists():
    for name, (b, thr, exact) in nc.normal_lists().items():
        keep = run_keep_list("NmsNormalGpu", b, thr, torch.int64)
        nc.judge_greedy(nc.normal_band(b), len(b), keep, op="gt", thr=thr)
        if exact:      # IoU exactly thr is not suppressed (>), one step above is, one step below is not
            sec = np.arange(1, len(b), 6)
            assert np.isin(sec, keep).all() and not np.isin(sec + 2, keep).any() and np.isin(sec + 4, keep).all()
        if name.startswith("chain"):
            np.testing.assert_array_equal(keep, np.concatenate([[0], np.arange(1, len(b), 2)]))


def test_circle_lists():
    for name, (xy, thr, exact) in nc.circle_lists().items():
        keep = run_circle(xy, thr)
        band = nc.circle_band(xy, exact=exact)
        nc.judge_greedy(band, len(xy), keep, op="le", thr=thr)
        if exact:      # squared distance exactly thresh suppresses (<=)
            np.testing.assert_array_equal(keep, nc.greedy_exact(band, len(xy), op="le", thr=thr))
            assert not np.isin(8 * np.arange(4) + 65, keep).any() and 8 * 4 + 65 in keep
        if name.startswith("chain"):
            np.testing.assert_array_equal(keep, np.concatenate([[0], np.arange(1, len(xy), 2)]))


# ------------------------------------------------------------------------------------------------ rotated
@pytest.mark.parametrize("name", sorted(nc.rot_lists()))
def test_rotated_lists(name):
    """NmsGpu (> thr, clamped union, int64 keep) and boxes_iou_nms_gpu (>= thr, no clamp, zero-area boxes dead, int32 keep) on
    clustered and chained car-sized boxes, on a list with CenterPoint's all-zero tail rows and on a list of dead boxes only."""
    b, thr = nc.rot_lists()[name]
    n = len(b)
    ov = nc.rot_overlap_matrix(b, b)
    k_gpu = run_keep_list("NmsGpu", b, thr, torch.int64)
    k_aot = run_keep_list("boxes_iou_nms_gpu", b, thr, torch.int32)
    nc.judge_greedy(nc.rot_band(b, "clamp", ov), n, k_gpu, op="gt", thr=thr)
    nc.judge_greedy(nc.rot_band(b, "none", ov), n, k_aot, dead=nc.rot_dead(b), op="ge", thr=thr)
    if name.startswith("chain"):
        np.testing.assert_array_equal(k_gpu, np.concatenate([[0], np.arange(1, n, 2)]))
        np.testing.assert_array_equal(k_aot, k_gpu)
    if name.startswith("tail"):       # zero rows: IoU 0 / 1e-8 = 0 among themselves for NmsGpu, dead for boxes_iou_nms_gpu
        assert np.isin(np.arange(n - 21, n), k_gpu).all() and not np.isin(np.arange(n - 21, n), k_aot).any()
    if name.startswith("dead-only"):
        assert len(k_aot) == 0


@pytest.mark.parametrize("thr", [0.5, 0.25])
def test_rotated_nested_ties(thr):
    """Overlap / union exactly thr (exact in fp32): NmsGpu (>) keeps the inner box, boxes_iou_nms_gpu (>=) drops it."""
    b = nc.rot_nested_ties(thr)
    sec = np.arange(1, len(b), 6)
    for sym, dtype, rule, op, tie_kept in (("NmsGpu", torch.int64, "clamp", "gt", True), ("boxes_iou_nms_gpu", torch.int32, "none", "ge", False)):
        keep = run_keep_list(sym, b, thr, dtype)
        nc.judge_greedy(nc.rot_band(b, rule), len(b), keep, dead=nc.rot_dead(b) if rule == "none" else None, op=op, thr=thr)
        assert np.isin(sec, keep).all() == tie_kept and np.isin(sec, keep).any() == tie_kept
        assert not np.isin(sec + 2, keep).any() and np.isin(sec + 4, keep).all() and np.isin(np.arange(0, len(b), 2), keep).all()


def test_bev_matrices_inside_their_bands():
    """BoxesOverlapBevGpu / BoxesIouBevGpu, 320 x 320 on the clustered list: every element inside the geometric band."""
    b, _ = nc.rot_lists()["clustered-320-0.7"]
    ov, iou = (call_twice(sym, [T(b), T(b)], [((320, 320), torch.float32)])[0].astype(np.float64) for sym in ("BoxesOverlapBevGpu", "BoxesIouBevGpu"))
    lo, hi = nc.with_rot_slack(*nc.rot_overlap_matrix(b, b))
    assert (hi > 0).sum() > 4000
    assert ((ov >= lo) & (ov <= hi)).all(), (np.max(lo - ov), np.max(ov - hi))
    area = (b[:, 3].astype(np.float64) * b[:, 4].astype(np.float64))
    vlo, vhi = nc.rot_iou_from_overlap(lo, hi, area[:, None], area[None, :], "clamp")
    assert ((iou >= vlo) & (iou <= vhi)).all(), (np.max(vlo - iou), np.max(iou - vhi))
    assert np.abs(np.diag(iou) - 1).max() < 0.02 and (iou[hi == 0] == 0).all()


# ------------------------------------------------------------------------------------------------ md_soft_nms
def run_soft(boxes, scores, count, method, threshold):
    from minddet_amd import det_ops

    L, n = boxes.shape[:2]
    inputs = [T(boxes.astype(np.float32)), T(scores.astype(np.float32)), None if count is None else T(np.asarray(count, np.int32))]
    return call_twice("md_soft_nms", inputs, [((L, n), torch.float32), ((L, n), torch.int32), ((L,), torch.int32)],
                      extra=det_ops._SoftNmsAttrs(0.5, 0.5, float(threshold), int(method)))


def check_soft(ref, so, order, num):
    k = len(ref["order"])
    assert int(num) == k
    np.testing.assert_array_equal(order[:k], ref["order"])            # the selection order, ties to the lower index
    assert (order[k:] == 0).all()
    np.testing.assert_array_equal(so > 0, ref["scores"] > 0)          # survivors; removed and absent boxes read 0
    err = np.abs(so.astype(np.float64) - ref["scores"])
    tol = nc.soft_tolerance(ref)
    worst = int(np.argmax(err - tol))
    assert (err <= tol).all(), (worst, so[worst], ref["scores"][worst], tol[worst], int(ref["ndecay"][worst]))


@pytest.mark.parametrize("case", nc.soft_cases(), ids=lambda c: "n%d-m%d-t%d" % (c[0], c[1], c[3]))
def test_soft_nms_order_and_scores(case):
    n, method, seed, ties, threshold = case
    boxes, scores, ref = nc.soft_nms_case(n, method, seed, ties, threshold)
    so, order, num = run_soft(boxes[None], scores[None], None, method, threshold)
    check_soft(ref, so[0], order[0], num[0])


@pytest.mark.parametrize("method", nc.SOFT_METHODS)
def test_soft_nms_batched_with_count(method):
    """L = 4 lists of 300 in one launch with count 300 / 0 / 65 / 1: boxes past a list's count are neither selected nor decay anything."""
    n, count = 300, [300, 0, 65, 1]
    cases = [nc.soft_nms_case(n, method, 8000 + 100 * l + method, 0, 0.001, count=c) for l, c in enumerate(count)]
    so, order, num = run_soft(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), count, method, 0.001)
    for l, c in enumerate(count):
        ref = cases[l][2]
        pad = dict(order=ref["order"], ndecay=np.pad(ref["ndecay"], (0, n - c)), scores=np.pad(ref["scores"], (0, n - c)), tol=np.pad(ref["tol"], (0, n - c)))
        check_soft(pad, so[l], order[l], num[l])
