"""GPU: the KITTI camera-frame ends (include/minddet_hip_kitti.h) through the C ABI, held to the float64 contract
(tests/kitti_io_contract.py).  The crop: keep, the order, offsets_out, every column of the kept rows and the zero tail exact -- on the
reference's own cases (tests/golden/kitti_io_vectors.npz; the planted rows by name), sample lengths around the workgroup width, an
empty sample in the middle, hull counts 0 / 1 / 3 / 64 and one above K, rows outside the offsets, a point count that takes the
block-count scan to its second pass, a sentinel-filled output, and the call forms.  The label boxes and the result rows: every stored
fp32 value equal to fp32(contract), at most 1 in 10^4 one ulp off, the kept set and src exact; M around the wave width, counts 0 / M /
above M, every filter alone and combined and off, a straddling box, a box behind the camera, a NaN row.  No case has an open decision
(the contract says so for each).  The chains on the tiny config: forward_kitti on a raw cloud against forward on the host-cropped one,
its rows against kitti_eval's host path within the derived bound, prepare_kitti + train_loss against host-converted inputs."""
import os

import numpy as np
import pytest
import torch

from tests import kitti_io_contract as kc
from tests.abi_cases_kitti import CASES
from tests.conftest import has_gpu
from tests.kitti_io_cases import CAR_RANGE, boxes_as_hulls, calibration, detections, fixture, scan
from tests.test_kitti_io_cpu import _host_annos, compare_annos, host_bounds

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_crop(pts, offsets, hulls, count, workspace=True, out=None):
    from minddet_amd import det_ops

    return det_ops.crop_hulls(dev(pts), dev(np.asarray(offsets, np.int32)), dev(hulls), dev(np.asarray(count, np.int32)), workspace=workspace, out=out)


def hold_crop(pts, offsets, hulls, count, what, **kw):
    """run, then the contract's check -> (the contract's dict, the outputs as numpy); the output starts as a sentinel the op must overwrite"""
    out = torch.full((len(pts), 4), -7.0, dtype=torch.float32, device=DEV)
    got = [x.cpu().numpy() for x in run_crop(pts, offsets, hulls, count, out=out, **kw)]
    c = kc.crop_hulls(pts, offsets, hulls, count)
    kc.check_crop(got[0], got[1], got[2], c, what)
    return c, got


@pytest.mark.parametrize("c", (0, 1))
def test_fixture_crops_against_the_contract_and_the_reference(c):
    z = fixture()
    pts, mask = z[f"cloud{c}"], z[f"rop{c}_mask"]
    cal = calibration((c,), DEV)
    from minddet_amd import det_ops

    out, offs, keep = (x.cpu().numpy() for x in det_ops.crop_hulls(dev(pts), dev(np.array([0, len(pts)], np.int32)), cal.image_frustum(), cal.tensor("image_count")))
    want = kc.crop_hulls(pts, [0, len(pts)], cal.image_frustum_host(), [1])
    kc.check_crop(out, offs, keep, want, f"image frustum {c}")
    assert np.array_equal(keep.astype(bool), mask) and kc.same_bits(out[:mask.sum()], pts[mask])          # remove_outside_points itself
    if c == 0:
        for row, name, kept in zip(z["plant_rows"], z["plant_names"], z["plant_mask"]):
            assert bool(keep[row]) == bool(kept), name
        hulls, count = cal.detection_frustums(z["det_bboxes"][None])
        for k in (3, 2):
            cnt = torch.full_like(count, k)
            out, offs, keep = (x.cpu().numpy() for x in det_ops.crop_hulls(dev(pts), dev(np.array([0, len(pts)], np.int32)), hulls, cnt))
            kc.check_crop(out, offs, keep, kc.crop_hulls(pts, [0, len(pts)], hulls.cpu().numpy(), [k]), f"detection frustums {k}")
            assert np.array_equal(keep.astype(bool), z["det_masks"][:, :k].any(-1))


def test_sample_lengths_around_the_workgroup_width_and_an_empty_middle_sample():
    rng = np.random.default_rng(21)
    lengths = [0, 1, 255, 256, 257, 513]
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    pts = scan(22, int(offsets[-1]), reach=45.0)
    hulls = boxes_as_hulls(rng, 6, 3)
    c, (out, offs, keep) = hold_crop(pts, offsets, hulls, [3] * 6, "lengths")
    assert 0.03 * len(pts) < offs[-1] < 0.7 * len(pts) and (np.diff(offs)[2:] > 0).all()
    offsets = [0, 400, 400, 900]
    c, (out, offs, keep) = hold_crop(pts[:900], offsets, hulls[:3], [3, 3, 2], "B = 3, the middle sample empty")
    assert offs[1] == offs[2] and 0 < offs[1] < offs[3]
    # rows before offsets[0] and from offsets[B] on belong to no sample: keep 0, not counted
    c, (out, offs, keep) = hold_crop(pts[:900], [37, 500, 810], hulls[:2], [3, 3], "rows outside the offsets")
    assert not keep[:37].any() and not keep[810:].any() and offs[0] == 0 and offs[2] == keep.sum() > 0
    inside_all = kc.crop_hulls(pts[:900], [0, 900], hulls[:1], [3])
    assert inside_all["keep"][:37].any() or inside_all["keep"][810:].any()                                 # (some of those rows do lie in a hull)


def test_hull_counts_zero_one_three_all_and_above_k():
    rng = np.random.default_rng(23)
    K = 64
    hulls = np.tile(boxes_as_hulls(rng, 1, K, span=40.0), (5, 1, 1, 1))       # the same hulls and the same points in every sample
    offsets = [0, 300, 600, 900, 1200, 1500]
    pts = np.tile(scan(24, 300, reach=50.0), (5, 1))
    counts = [0, 1, 3, 64, 70]
    c, (out, offs, keep) = hold_crop(pts, offsets, hulls, counts, "hull counts")
    n = np.diff(offs)
    assert n[0] == 0 and n[1] <= n[2] < n[3] == n[4] and n[2] > 0
    clamped = kc.crop_hulls(pts, offsets, hulls, [0, 1, 3, 64, 64])
    assert np.array_equal(clamped["keep"], c["keep"])                                                     # a count above K is K
    neg = hold_crop(pts, offsets, hulls, [-3, 1, 3, 64, 64], "a negative count")[1]
    assert kc.same_bits(neg[0], out)
    last = kc.inside(pts[1200:], hulls[4])[0]
    assert (last[:, 40:].any(1) & ~last[:, :40].any(1)).any()                                             # the late hulls decide some points


def test_block_count_scan_second_pass():
    """257 workgroups of points: one more than a pass of the one-workgroup scan over the block counts holds (256 x 256 + 1 rows)"""
    cal = calibration((0,), DEV)
    pts = scan(25, 256 * 256 + 1)
    c, (out, offs, keep) = hold_crop(pts, [0, len(pts)], cal.image_frustum_host(), [1], "257 blocks")
    assert 0.1 * len(pts) < offs[1] < 0.4 * len(pts) and c["src"][-1] >= 256 * 256 - 64 and not out[offs[1]:].any()


def test_bit_identical_across_calls_streams_and_call_forms():
    rng = np.random.default_rng(26)
    pts, offsets = scan(27, 1700, reach=45.0), [0, 700, 1213, 1700]
    hulls, count = boxes_as_hulls(rng, 3, 5), [5, 2, 4]
    first = run_crop(pts, offsets, hulls, count)
    again = run_crop(pts, offsets, hulls, count)
    pool = run_crop(pts, offsets, hulls, count, workspace=False)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = run_crop(pts, offsets, hulls, count)
        pool_side = run_crop(pts, offsets, hulls, count, workspace=False)
    torch.cuda.synchronize()
    assert int(first[1][-1]) > 50
    for tag, o in (("again", again), ("pool", pool), ("second stream", other), ("pool on the second stream", pool_side)):
        for a, b in zip(first, o):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), tag


def test_label_boxes_to_lidar():
    from minddet_amd import det_ops

    z = fixture()
    cal = calibration((0, 1), DEV)
    lab = np.stack([z["lab0_cam"], z["lab1_cam"]])
    total = 0
    for count in ([24, 24], [24, 5], [0, 30], [-2, 1]):
        got = det_ops.kitti_boxes_to_lidar(dev(lab), dev(np.array(count, np.int32)), cal.tensor("cam2lidar")).cpu().numpy()
        want, _ = kc.boxes_to_lidar(lab, count, cal.cam2lidar)
        differ, n = kc.check_stored(got, want, f"count {count}")
        total += differ
        live = np.arange(24)[None] < np.clip(count, 0, 24)[:, None]
        assert kc.same_bits(got[..., 3:], want[..., 3:]) and not got[~live].any()
    ref = np.stack([z["lab0_lidar"], z["lab1_lidar"]]).astype(np.float32)
    got = det_ops.kitti_boxes_to_lidar(dev(lab), dev(np.array([24, 24], np.int32)), cal.tensor("cam2lidar")).cpu().numpy()
    assert kc.ulp_steps(got, ref).max() <= 1 and total == 0                                               # the reference's own fp32 result: one ulp at most


def mixed_detections(seed, B, M, cal):
    """detections with every way out among them: to the left and right of the image, beyond the range in x and z, behind the camera"""
    d = detections(seed, B, M, cal, spread=4.5)
    rng = np.random.default_rng(seed + 1000)
    pick = rng.uniform(0, 1, (B, M))
    d[..., 0] = np.where(pick < 0.1, d[..., 0] * np.float32(1.6), d[..., 0])
    d[..., 2] = np.where((pick >= 0.1) & (pick < 0.15), np.float32(5.5), d[..., 2])
    d[..., 0] = np.where((pick >= 0.15) & (pick < 0.22), -d[..., 0], d[..., 0])
    return d


def hold_rows(dets, count, cal, limit, lidar_input, what):
    from minddet_amd import det_ops

    rows, src, out_count = (x.cpu().numpy() for x in det_ops.kitti_rows(dev(dets), dev(np.asarray(count, np.int32)), cal.tensor("lidar2cam"), cal.tensor("p2"),
                                                                         cal.tensor("image_shape"), limit_range=limit, lidar_input=lidar_input))
    c = kc.kitti_rows(dets, count, cal.lidar2cam, cal.p2, cal.image_shape, limit, lidar_input)
    differ, total = kc.check_rows(rows, src, out_count, c, what)
    n = c["count"]
    for b in range(len(dets)):
        assert not rows[b, n[b]:].any() and (src[b, n[b]:] == -1).all(), what                            # the zero rows behind the survivors
        kept = src[b, :n[b]]
        assert kc.same_bits(rows[b, :n[b]][:, [5, 6, 7, 11, 12, 13]], dets[b, kept][:, [4, 5, 3, 6, 7, 8]]), what      # passed through bit for bit
    return c, rows, differ, total


@pytest.mark.parametrize("M", (1, 63, 64, 65, 300))
def test_rows_around_the_wave_width_with_every_count(M):
    cal = calibration((0, 1, 0), DEV)
    dets = mixed_detections(30 + M, 3, M, cal)
    c, rows, differ, total = hold_rows(dets, [0, M, M + 5], cal, CAR_RANGE, False, f"M = {M}")
    assert c["count"][0] == 0 and c["count"][1] <= M
    if M >= 63:
        assert 0 < c["count"][1] < M and c["dropped"][1].sum() >= 5 and differ <= kc.FEW * total
    part = hold_rows(dets, [0, M // 2, 1], cal, CAR_RANGE, False, f"M = {M}, part")[0]
    assert part["count"][1] <= M // 2 and (part["src"][2, 1:] == -1).all()


def test_rows_filters_alone_combined_and_off():
    cal = calibration((0, 1), DEV)
    dets = mixed_detections(41, 2, 120, cal)
    dets[0, 3, :3] = (6.0, 3.2, -1.0)                                       # straddles the left border of the image
    dets[1, 4, :3] = (-20.0, 1.0, -1.0)                                     # behind the camera
    dets[1, 9, 0] = np.nan
    dets[0, 11, 6] = np.nan
    counts = {}
    for limit, lidar_input in ((CAR_RANGE, False), (None, False), (CAR_RANGE, True), (None, True)):
        c, rows, _, _ = hold_rows(dets, [120, 120], cal, limit, lidar_input, f"{limit is not None} {lidar_input}")
        counts[(limit is not None, lidar_input)] = int(c["count"].sum())
        for b, m in ((1, 9), (0, 11)):                                      # a NaN compares false everywhere: the row is reported, NaN through
            at = np.flatnonzero(c["src"][b] == m)
            assert len(at) == 1 and np.isnan(rows[b, at[0], 0])
        if not lidar_input:
            at = int(np.flatnonzero(c["src"][0] == 3)[0])
            assert rows[0, at, 1] == 0.0 and rows[0, at, 3] > 0 and c["rows"][0, at, 3] <= cal.image_shape[0, 1]      # clipped, kept
        assert (c["src"][1] == 4).any() == (not c["dropped"][1, 4]) and (limit is None or c["dropped"][1, 4]) and (limit is not None or not lidar_input or not c["dropped"][1, 4])
    assert counts[(False, True)] == 240 and counts[(True, False)] < counts[(True, True)] < 240 and counts[(True, False)] < counts[(False, False)] < 240
    # one-sided limits: each comparison alone
    inf = float("inf")
    for k in range(6):
        lim = [-inf] * 3 + [inf] * 3
        lim[k] = CAR_RANGE[k]
        c = hold_rows(dets, [120, 120], cal, lim, True, f"limit {k} alone")[0]
        col = dets[..., k % 3].astype(np.float64)
        with np.errstate(invalid="ignore"):
            want = (col < np.float32(lim[k])) if k < 3 else (col > np.float32(lim[k]))
        assert np.array_equal(c["dropped"], want) and (k in (1, 2) or want.any())


def _model():
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", "pointpillars_tiny_kitti.py"))
    aug = dict(gt_loc_noise_std=[0.1, 0.1, 0.05], gt_rotation_noise=[-0.2, 0.2], global_rotation_noise=[-0.1, 0.1],
               global_scaling_noise=[0.97, 1.03], global_loc_noise_std=[0.05, 0.05, 0.05], global_random_rot_range=[-0.05, 0.05], num_try=20)
    return build_detector(dict(cfg.model), dict(augment=aug), cfg.test_cfg).to(DEV), cfg


def _raw_scans():
    """two raw scans around the sensor within the tiny range's reach, full turn; offsets"""
    a, b = scan(50, 3000, reach=8.0, zlo=-1.8, zhi=0.4), scan(51, 2300, reach=8.0, zlo=-1.8, zhi=0.4)
    return np.concatenate([a, b]), np.array([0, 3000, 5300], np.int32)


def test_chain_forward_kitti_equals_forward_on_the_host_cropped_cloud():
    from minddet_amd import kitti_eval

    m, cfg = _model()
    cal = calibration((0, 1), DEV)
    pts, offsets = _raw_scans()
    want = kc.crop_hulls(pts, offsets, cal.image_frustum_host(), [1, 1])
    assert not want["open"].any() and 300 < want["offsets"][1] < 2000 and want["offsets"][2] - want["offsets"][1] > 200
    rows, src, out_count, dets = m.forward_kitti(dev(pts), dev(offsets), cal)
    dets2, count2 = m.forward(dev(want["points"]), dev(want["offsets"]))
    assert torch.equal(dets.view(torch.int32), dets2.view(torch.int32)) and int(count2.min()) > 3
    # the rows against the host path on the same dets
    d, n = dets.cpu().numpy(), count2.cpu().numpy()
    limit = cfg.test_cfg["post_center_limit_range"]
    c = kc.kitti_rows(d, n, cal.lidar2cam, cal.p2, cal.image_shape, limit, False)
    differ, total = kc.check_rows(rows.cpu().numpy(), src.cpu().numpy(), out_count.cpu().numpy(), c, "tiny config")
    bounds = host_bounds(d, c, cal)
    for b in range(2):                                                      # no decision of the host path lies within the bound of its threshold
        live = np.arange(d.shape[1]) < n[b]
        lim = np.asarray(limit, np.float32).astype(np.float64)
        in_range = live & ~((d[b, :, :3] < lim[:3]).any(1) | (d[b, :, :3] > lim[3:]).any(1))
        g = kc.camera_rows(d[b, in_range], cal.lidar2cam[b], cal.p2[b])
        bb, _ = kc.host_path_bound(d[b, in_range], cal.lidar2cam[b], cal.p2[b])
        H, W = cal.image_shape[b]
        gap = np.abs(g["bbox"] - np.array([W, H, 0, 0]))
        assert (gap > bb).all(), ("a decision within the host path's bound", b, (gap - bb).min())
    names = list(m.class_names)
    got = kitti_eval.rows_to_annos(rows, src, out_count, dets, names, [100, 101])
    annos = _host_annos(d, n, cal, limit, False, names)
    compare_annos(got, annos, bounds, "tiny config")
    assert sum(len(a["name"]) for a in got) > 0
    text = kitti_eval.kitti_result_lines(got[0]) + kitti_eval.kitti_result_lines(got[1])
    assert len(text) == int(out_count.sum())


def test_chain_prepare_kitti_and_train_loss_equal_host_converted_inputs():
    m, cfg = _model()
    cal = calibration((0, 1), DEV)
    pts, offsets = _raw_scans()
    rng = np.random.default_rng(52)
    B, G = 2, 4
    lidar = np.zeros((B, G, 7))
    for b in range(B):
        for g in range(G):
            lidar[b, g] = (2.0 + 1.3 * g, rng.uniform(-1.5, 1.5), rng.uniform(-1.6, -1.2), 0.6, rng.choice([0.8, 1.76]), 1.73, rng.uniform(-1, 1))
    cam = np.concatenate([kc.apply4(cal.lidar2cam, lidar[..., :3]), lidar[..., [4, 5, 3, 6]]], -1).astype(np.float32)      # (x, y, z, l, h, w, r)
    count = np.array([4, 3], np.int32)
    classes = dev(np.tile(np.array([[1, 2, 1, 2]], np.int32), (B, 1)))
    bboxes = np.array([[[0.0, 0, 700, 375], [650, 0, 1242, 375]], [[0.0, 0, 1224, 370], [0, 0, 1, 1]]])
    # the device chain
    p1, o1, boxes1 = m.prepare_kitti(dev(pts), dev(offsets), cal, gt_boxes_camera=dev(cam), gt_count=dev(count), reference_detections=(bboxes, [2, 1]))
    # the same on the host: the detection frustums first, then the image frustum
    hulls, hcount = cal.detection_frustums_host(bboxes, [2, 1])
    first = kc.crop_hulls(pts, offsets, hulls, hcount)
    second = kc.crop_hulls(first["points"], first["offsets"], cal.image_frustum_host(), [1, 1])
    assert not first["open"].any() and not second["open"].any() and 0 < second["offsets"][-1] <= first["offsets"][-1] < len(pts)
    want_boxes, _ = kc.boxes_to_lidar(cam, count, cal.cam2lidar)
    assert kc.same_bits(p1.cpu().numpy(), second["points"]) and np.array_equal(o1.cpu().numpy(), second["offsets"])
    kc.check_stored(boxes1.cpu().numpy(), want_boxes, "label boxes")
    assert kc.same_bits(boxes1.cpu().numpy(), want_boxes)                  # (no value of this case sits on an fp32 boundary)
    assert np.abs(want_boxes[0, :, :3] - lidar[0, :, :3]).max() < 1e-5     # there and back
    draws = m.augment_op().draw(boxes1, dev(count), torch.Generator(device=DEV).manual_seed(5))
    one = m.train_loss(p1, o1, boxes1, classes, dev(count), draws=draws)
    two = m.train_loss(dev(second["points"]), dev(second["offsets"]), dev(want_boxes), classes, dev(count), draws=draws)
    torch.cuda.synchronize()
    for k in ("total", "parts", "num_pos"):
        assert torch.isfinite(one[k].float()).all() and torch.equal(one[k].view(torch.uint8), two[k].view(torch.uint8)), k
    assert float(one["total"]) > 0
    # without reference detections and labels: the image frustum alone
    p2_, o2_, none = m.prepare_kitti(dev(pts), dev(offsets), cal)
    img = kc.crop_hulls(pts, offsets, cal.image_frustum_host(), [1, 1])
    assert none is None and kc.same_bits(p2_.cpu().numpy(), img["points"]) and np.array_equal(o2_.cpu().numpy(), img["offsets"])


def test_abi_rows_are_accepted():
    from minddet_amd import _lib

    dt = {"float32": torch.float32, "float64": torch.float64, "int32": torch.int32, "uint8": torch.uint8}
    keep = []
    for c in CASES:
        tensors = [torch.zeros(t.shape, dtype=dt[t.dtype], device=DEV) for t in c.operands]
        n_in = {"md_pc_crop_hulls": 4, "md_kitti_boxes_to_lidar": 3, "md_kitti_rows": 5}[c.sym]
        for t in tensors[n_in:]:
            t.fill_(3)                                                     # the outputs start as a sentinel
        keep.append((c, n_in, tensors))
        assert _lib.call(c.sym, tensors, extra=c.extra) == 0, c.id
    torch.cuda.synchronize()
    for c, n_in, tensors in keep:                                          # zero offsets and counts: nothing is kept, every output is written
        outs = tensors[n_in:n_in + 3] if c.sym != "md_kitti_boxes_to_lidar" else tensors[3:4]
        if c.sym == "md_kitti_rows":
            assert not outs[0].any() and (outs[1] == -1).all() and not outs[2].any(), c.id
        else:
            for t in outs:
                assert not t.any(), c.id
