"""GPU: the KITTI training augmentation (include/minddet_hip_pcaug.h) through the C ABI -- parity with the reference's own outputs
(tests/golden/pc_augment_vectors.npz) on every decided decision and with the float64 contract (tests/pcaug_contract.py) on the
values, the collision predicate on the 40 planted pairs, a batch with an empty sample, straddling blocks and a sample without ground
truth, determinism and the call forms, the chain into md_voxelize / md_assign_targets / the loss, the draws, and the ABI rows.

The rule for fp32 outputs is the one of the training losses: within 1 ulp of the contract's rounded value, at most 1 in 10^4
differing at all.  obj_transform (float64): within 4 float64 ulp of the contract."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import pcaug_contract as pc
from tests.conftest import has_gpu
from tests.pcaug_cases import NAMES, contract_case, fixture_case, reference_owner

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def to_np(t):
    return {k: v.cpu().numpy() for k, v in t.items()}


def case_inputs(name):
    f = fixture_case(name)
    G, N, R = len(f["gt_boxes"]), len(f["points"]), len(f["remove_boxes"])
    d = dict(points=dev(f["points"]), offsets=dev(np.array([0, N], np.int32)), gt_boxes=dev(f["gt_boxes"][None]),
             gt_count=dev(np.array([G], np.int32)), valid=dev(f["valid"][None]), classes=dev(f["classes"][None]),
             loc=dev(f["loc"][None]), rot=dev(f["rot"][None]), grot=dev(f["grot"][None]) if "grot" in f else None, glob=dev(f["global"][None]))
    if R:
        d.update(remove_boxes=dev(f["remove_boxes"][None]), remove_count=dev(np.array([R], np.int32)),
                 remove_from=dev(np.array([int(f["remove_from"])], np.int32)))
    return d


def run_ops(d, bv_range, workspace=True):
    from minddet_amd import det_ops

    sel, tf, moved = det_ops.pc_noise_per_object(d["gt_boxes"], d["gt_count"], d["valid"], d["loc"], d["rot"], d["grot"])
    pts, offs, owner = det_ops.pc_augment_points(d["points"], d["offsets"], d["gt_boxes"], d["gt_count"], d["valid"], tf, d["glob"],
                                                 d.get("remove_boxes"), d.get("remove_count"), d.get("remove_from"), workspace=workspace)
    boxes, classes, count = det_ops.pc_augment_boxes(moved, d["gt_count"], d["valid"], d["classes"], d["glob"], bv_range)
    return dict(selected=sel, obj_transform=tf, boxes_out=moved, points=pts, offsets=offs, owner=owner, gt_boxes=boxes, gt_classes=classes,
                gt_count=count)


@functools.lru_cache(maxsize=None)
def device_case(name):
    out = to_np(run_ops(case_inputs(name), fixture_case(name)["bv_range"]))
    torch.cuda.synchronize()
    return out


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
    assert worst <= 1.0 and frac <= max(few, 0.0), (what, worst, frac)


def check_against_contract(tag, got, sel, tf, moved, pts, boxes, n_points):
    """one sample of the device's result against the contract's (see contract_case)"""
    assert np.array_equal(got["selected"], sel), tag
    err = np.abs(got["obj_transform"] - tf) / np.spacing(np.maximum(np.abs(tf), 1e-300))
    print(f"{tag}: obj_transform worst {err.max() if err.size else 0:.2f} float64 ulp")
    assert err.size == 0 or err.max() <= 4.0, (tag, float(err.max()))
    check32(tag + " boxes_out", got["boxes_out"], moved)
    d = pts["decided"]
    assert np.array_equal(got["owner"][d], pts["owner"][d]), tag
    same = np.array_equal(got["owner"], pts["owner"])
    if d.all() or same:
        assert got["offsets"][1] - got["offsets"][0] == len(pts["points"]), tag
    if same:
        k = len(pts["points"])
        check32(tag + " points", got["points"][:k, :3], pts["points"][:, :3])
        assert np.array_equal(got["points"][:k, 3], pts["points"][:, 3]) and not got["points"][k:n_points].any(), tag
    dec = boxes["margin"] > pc.MARGIN
    if dec.all():
        assert int(got["gt_count"]) == boxes["count"] and np.array_equal(got["gt_classes"], boxes["gt_classes"]), tag
        check32(tag + " gt_boxes", got["gt_boxes"], boxes["gt_boxes"])
    return same


@pytest.mark.parametrize("name", NAMES)
def test_parity_with_the_reference_and_the_contract(name):
    f, c, got = fixture_case(name), contract_case(name), device_case(name)
    one = {k: (v[0] if k in ("selected", "obj_transform", "boxes_out", "gt_boxes", "gt_classes", "gt_count") else v) for k, v in got.items()}
    # the reference's own decisions
    assert np.array_equal(one["selected"], f["selected"])
    n = len(f["points"])
    own_ref = reference_owner(f)
    d = c["pts"]["decided"]
    assert np.array_equal(one["owner"][d], own_ref[d])
    assert not d.all() and c["pts"]["drop_decided"]          # the plants sit on ground-truth boxes' faces, none on a remove box: the kept count is decided
    assert one["offsets"].tolist() == [0, len(f["points_translate"])] and np.array_equal(one["owner"] == -2, own_ref == -2)
    mask_ref = np.zeros(len(f["valid"]), bool)
    mask_ref[np.flatnonzero(f["valid"])] = f["range_mask"]
    if (c["boxes"]["margin"] > pc.MARGIN).all():
        assert int(one["gt_count"]) == int(mask_ref.sum()) and np.array_equal(one["gt_classes"][:int(one["gt_count"])], f["final_classes"])
    assert check_against_contract(name, one, c["selected"], c["tf"], c["moved"], c["pts"], c["boxes"], n)
    # the all-collide boxes and the invalid ones keep their rows, and their points do not move before the global steps
    for g in np.flatnonzero(one["selected"] < 0):
        assert np.array_equal(one["boxes_out"][g], f["gt_boxes"][g]) and not one["obj_transform"][g].any()
    if name == "car":
        assert one["selected"][0] == -1 and one["selected"][7] == -1 and (one["owner"] == 0).any()
        idx = np.flatnonzero(one["owner"] == 0)
        alone = pc.augment_points(f["points"][idx], f["gt_boxes"], 0, f["valid"], c["tf"], f["global"])    # no box at all: the global steps only
        at = np.flatnonzero(one["owner"] != -2).searchsorted(idx)
        check32("car: points of the box that stays", one["points"][at, :3], alone["points"][:, :3])


def test_collision_predicate_on_the_planted_pairs():
    from minddet_amd import det_ops

    z = np.load(os.path.join(ROOT, "tests", "golden", "pc_augment_vectors.npz"))
    A, Bq = z["collision_a"], z["collision_b"]
    boxes = np.zeros((40, 2, 7), np.float32)
    for k, src in enumerate((Bq, A)):                      # row 0: B, not valid, stays; row 1: A with a zero try
        boxes[:, k, 0:2], boxes[:, k, 3:5], boxes[:, k, 6], boxes[:, k, 5] = src[:, 0:2], src[:, 2:4], src[:, 4], 1.5
    valid = np.tile(np.array([[0, 1]], np.uint8), (40, 1))
    sel, tf, moved = det_ops.pc_noise_per_object(dev(boxes), dev(np.full(40, 2, np.int32)), dev(valid), torch.zeros((40, 2, 1, 3), dtype=torch.float64,
                                                 device=DEV), torch.zeros((40, 2, 1), dtype=torch.float64, device=DEV), None)
    want = z["collision_standup"] & (z["collision_edges"] | z["collision_a_covers_b"] | z["collision_b_covers_a"])
    sel = sel.cpu().numpy()
    assert (sel[:, 0] == -1).all() and np.array_equal(sel[:, 1] == -1, want), (sel[:, 1].tolist(), want.tolist())
    assert want.sum() == 24 and torch.equal(moved.cpu(), torch.from_numpy(boxes))


def test_crowded_scenes_select_the_contracts_tries():
    """40 boxes on 14 m x 14 m per sample: most first tries collide, so later tries win (some in the second wave, >= 64), many boxes
    find none, and each box is tested against where the earlier ones ended up; both forms, against the float64 contract"""
    from minddet_amd import det_ops

    rng = np.random.default_rng(21)
    B, G, T = 3, 40, 100
    boxes = np.zeros((B, G, 7), np.float32)
    boxes[..., 0], boxes[..., 1], boxes[..., 2] = rng.uniform(10, 24, (B, G)), rng.uniform(-7, 7, (B, G)), -1.5
    boxes[..., 3], boxes[..., 4], boxes[..., 5] = rng.uniform(0.6, 1.9, (B, G)), rng.uniform(0.8, 4.6, (B, G)), 1.6
    boxes[..., 6] = rng.uniform(-3, 3, (B, G))
    loc, rot, grot = rng.normal(0, 0.6, (B, G, T, 3)), rng.uniform(-0.5, 0.5, (B, G, T)), rng.uniform(-0.02, 0.02, (B, G, T))
    valid = np.ones((B, G), np.uint8)
    valid[0, 5] = valid[2, 0] = 0
    count = np.array([40, 33, 40], np.int32)
    for form, gr in (("v2", grot), ("plain", None)):
        sel, tf, moved = (t.cpu().numpy() for t in det_ops.pc_noise_per_object(dev(boxes), dev(count), dev(valid), dev(loc), dev(rot),
                                                                               None if gr is None else dev(gr)))
        for b in range(B):
            w_sel, w_tf, w_moved = pc.noise_per_object(boxes[b], int(count[b]), valid[b], loc[b], rot[b], None if gr is None else gr[b])
            assert np.array_equal(sel[b], w_sel), (form, b, sel[b].tolist(), w_sel.tolist())
            err = np.abs(tf[b] - w_tf) / np.spacing(np.maximum(np.abs(w_tf), 1e-300))
            print(f"crowded {form} sample {b}: tries {sorted(set(w_sel.tolist()))[-4:]}, none {(w_sel < 0).sum()}, obj_transform worst {err.max():.2f} ulp")
            assert err.max() <= 4.0
            check32(f"crowded {form} sample {b} boxes_out", moved[b], w_moved)
        assert (sel >= 64).any() and (sel > 0).sum() >= 20 and (sel[:, :33] < 0).sum() >= 20 and (sel[1, 33:] == -1).all()


def batch3(sizes=(0, 300, 2050)):
    """B = 3: an empty sample, 300 and 2 050 points (blocks that straddle samples, several blocks per sample), the empty sample without
    ground truth; G = 6, T = 7, R = 2"""
    rng = np.random.default_rng(5)
    G, T, R = 6, 7, 2
    boxes = np.zeros((3, G, 7), np.float32)
    for b in range(3):
        for g in range(G):
            boxes[b, g] = (8 + 9 * g + rng.uniform(-1, 1), rng.uniform(-20, 20), -1.5, 1.6, 3.9, 1.6, rng.uniform(-3, 3))
    count = np.array([0, 6, 5], np.int32)
    valid = np.ones((3, G), np.uint8)
    valid[1, 2] = 0
    pts = []
    for b, n in enumerate(sizes):
        inside = boxes[b, rng.integers(0, G, n), :3] + rng.uniform(-1.2, 1.2, (n, 3)) + (0, 0, 0.8)
        bg = np.stack([rng.uniform(0, 69, n), rng.uniform(-39, 39, n), rng.uniform(-2.5, 0.5, n)], 1)
        xyz = np.where((rng.uniform(size=n) < 0.6)[:, None], inside, bg)
        pts.append(np.concatenate([xyz, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32))
    rem = np.zeros((3, R, 7), np.float32)
    for b in range(3):
        for r in range(R):
            rem[b, r] = (rng.uniform(10, 60), rng.uniform(-30, 30), -2.0, 8.0, 12.0, 2.5, rng.uniform(-3, 3))
    glob = np.array([[1, 0.3, 1.02, 0.1, -0.2, 0.05], [0, -0.5, 0.97, -0.3, 0.1, 0.0], [1, 0.7, 1.04, 0.2, 0.2, -0.1]], np.float64)
    return dict(points=pts, boxes=boxes, count=count, valid=valid, classes=(1 + np.arange(3 * G).reshape(3, G) % 2).astype(np.int32),
                loc=rng.normal(0, 0.25, (3, G, T, 3)), rot=rng.uniform(-0.15, 0.15, (3, G, T)), grot=rng.uniform(-0.05, 0.05, (3, G, T)), glob=glob,
                rem=rem, rem_count=np.array([2, 1, 2], np.int32), rem_from=np.array([0, 40, 100], np.int32), bv=(0.0, -39.68, 69.12, 39.68))


def batch3_inputs(s):
    offs = np.concatenate([[0], np.cumsum([len(p) for p in s["points"]])]).astype(np.int32)
    return dict(points=dev(np.concatenate(s["points"])), offsets=dev(offs), gt_boxes=dev(s["boxes"]), gt_count=dev(s["count"]),
                valid=dev(s["valid"]), classes=dev(s["classes"]), loc=dev(s["loc"]), rot=dev(s["rot"]), grot=dev(s["grot"]), glob=dev(s["glob"]),
                remove_boxes=dev(s["rem"]), remove_count=dev(s["rem_count"]), remove_from=dev(s["rem_from"])), offs


def check_batch3(s):
    d, offs = batch3_inputs(s)
    got = to_np(run_ops(d, s["bv"]))
    assert got["offsets"][0] == 0 and (np.diff(got["offsets"]) >= 0).all() and got["offsets"][1] == 0
    total = int(got["offsets"][3])
    assert not got["points"][total:].any() and (got["owner"] == -2).sum() == len(got["owner"]) - total > 0
    for b in range(3):
        cnt = int(s["count"][b])
        sel, tf, moved = pc.noise_per_object(s["boxes"][b], cnt, s["valid"][b], s["loc"][b], s["rot"][b], s["grot"][b])
        pts = pc.augment_points(s["points"][b], s["boxes"][b], cnt, s["valid"][b], tf, s["glob"][b], s["rem"][b], int(s["rem_count"][b]),
                                int(s["rem_from"][b]))
        boxes = pc.augment_boxes(moved, cnt, s["valid"][b], s["classes"][b], s["glob"][b], s["bv"])
        one = dict(selected=got["selected"][b], obj_transform=got["obj_transform"][b], boxes_out=got["boxes_out"][b],
                   owner=got["owner"][offs[b]:offs[b + 1]], offsets=got["offsets"][b:b + 2],
                   points=got["points"][got["offsets"][b]:got["offsets"][b + 1]], gt_boxes=got["gt_boxes"][b], gt_classes=got["gt_classes"][b],
                   gt_count=got["gt_count"][b])
        same = check_against_contract(f"sample {b}", one, sel, tf, moved, pts, boxes, len(pts["points"]))
        assert same or not pts["decided"].all()
        if b == 0:
            assert (one["selected"] == -1).all() and not one["gt_boxes"].any() and int(one["gt_count"]) == 0 and (one["owner"] < 0).all()
    return got, offs


def test_batch_with_an_empty_sample_and_straddling_blocks():
    got, offs = check_batch3(batch3())
    assert (got["owner"][offs[1]:offs[2]] >= 0).any() and (got["selected"][1] >= 0).sum() >= 4


def test_compaction_with_more_block_counts_than_one_scan_pass():
    """256 * 256 + 1 points: 257 block counts, so the one-workgroup scan of the counts takes a second pass and carries the first's total"""
    s = batch3(sizes=(0, 300, 256 * 256 + 1 - 300))
    got, offs = check_batch3(s)
    total = int(got["offsets"][3])
    assert len(got["owner"]) == 256 * 256 + 1 and total > 256 * 128
    # every kept row's place, whatever the contract left undecided: the fourth column is copied, so it names the row
    assert np.array_equal(got["points"][:total, 3], np.concatenate(s["points"])[got["owner"] != -2, 3])


def test_determinism_and_call_forms():
    d = case_inputs("pedcyc")
    bv = fixture_case("pedcyc")["bv_range"]
    first = run_ops(d, bv)
    again = run_ops(d, bv)
    pool = run_ops(d, bv, workspace=False)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = run_ops(d, bv)
    torch.cuda.synchronize()
    for k, v in first.items():
        raw = v.view(torch.uint8)
        for tag, o in (("again", again), ("pool", pool), ("second stream", other)):
            assert torch.equal(raw, o[k].view(torch.uint8)), (k, tag)
    want = device_case("pedcyc")
    assert all(np.array_equal(first[k].cpu().numpy(), want[k]) for k in want)


def _model():
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", "pointpillars_tiny_points.py"))
    aug = dict(gt_loc_noise_std=[0.1, 0.1, 0.05], gt_rotation_noise=[-0.2, 0.2], global_rotation_noise=[-0.1, 0.1],
               global_scaling_noise=[0.97, 1.03], global_loc_noise_std=[0.05, 0.05, 0.05], global_random_rot_range=[-0.05, 0.05], num_try=20)
    return build_detector(dict(cfg.model), dict(augment=aug), cfg.test_cfg).to(DEV)


def test_chain_into_voxeliser_targets_and_loss():
    from minddet_amd import det_ops
    from tests.test_pp_reader_gpu import small_cloud

    m = _model()
    B, G = 3, 6
    pts, offs = small_cloud(m, B, 1200, 3)
    rng = np.random.default_rng(8)
    anchors = m.inner.anchors.cpu().numpy()
    boxes = np.zeros((B, G, 7), np.float32)
    for b in range(B):                                     # ground truth on top of anchors, apart from each other
        pick = rng.choice(len(anchors) // 4, G, replace=False) * 4
        boxes[b] = anchors[pick]
        boxes[b, :, :2] += 0.03
    count = np.array([6, 0, 4], np.int32)
    classes = np.tile(np.array([[1, 2, 1, 2, 1, 2]], np.int32), (B, 1))
    args = (dev(pts), dev(offs), dev(boxes), dev(classes), dev(count))
    aug = m.augment_op()
    assert aug.enable_grot and aug.num_try == 20
    draws = aug.draw(args[2], args[4], torch.Generator(device=DEV).manual_seed(3))
    # sampled objects' boxes: points inside them are dropped from remove_from on, so the compaction moves rows and leaves zero rows behind
    rem = np.zeros((B, 2, 7), np.float32)
    rem[:, 0], rem[:, 1] = (2.0, -1.0, -2.4, 1.8, 1.6, 2.8, 0.4), (5.5, 1.2, -2.4, 1.5, 2.0, 2.8, -0.9)
    sampled = dict(remove_boxes=dev(rem), remove_count=dev(np.array([2, 1, 2], np.int32)), remove_from=dev(np.array([0, 100, 50], np.int32)))
    ex = m.train_example(*args, draws=draws, sampled=sampled)
    a = ex["augment"]
    # md_voxelize on the op's compacted points (N rows, zero rows behind the last kept one) == md_voxelize on the kept rows alone,
    # put together on the host sample by sample from the owners
    p_np, o_np, owner = a["points"].cpu().numpy(), a["offsets"].cpu().numpy(), a["owner"].cpu().numpy()
    kept = np.array([int((owner[offs[b]:offs[b + 1]] != -2).sum()) for b in range(B)])
    assert (kept < 1200).all() and (kept > 600).all() and o_np.tolist() == [0] + np.cumsum(kept).tolist() and (owner >= 0).any()
    assert o_np[-1] < len(p_np) and not p_np[o_np[-1]:].any() and p_np[:o_np[-1], :3].any(1).all()
    host = np.concatenate([p_np[o_np[b]:o_np[b + 1]] for b in range(B)])
    assert len(host) == o_np[-1] < len(pts)
    vox_a = det_ops.voxelize(a["points"], a["offsets"], m.voxel_size, m.pc_range, m.max_points, m.max_voxels)
    vox_b = det_ops.voxelize(dev(host), dev(o_np), m.voxel_size, m.pc_range, m.max_points, m.max_voxels)
    for x, y in zip(vox_a, vox_b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # the targets of the fixed-capacity list == det_ops.assign_targets on the host-sliced list of each sample
    n_out = a["gt_count"].cpu().numpy()
    assert n_out[1] == 0 and n_out[0] >= 1
    gen = det_ops.generate_anchors(m.inner.generators, (1,) + tuple(m.inner.feature_hw), device=DEV)
    for b in range(B):
        n = int(n_out[b])
        want = det_ops.assign_targets(m.inner.anchors, a["gt_boxes"][b, :n].contiguous(), a["gt_classes"][b, :n].contiguous(),
                                      gen["matched_thresholds"], gen["unmatched_thresholds"], ex["anchors_mask"][b])
        for k, w in zip(("labels", "reg_targets", "reg_weights"), want):
            assert torch.equal(ex[k][b].view(torch.int32), w.view(torch.int32)), (b, k)
    one = m.train_loss(*args, draws=draws, sampled=sampled, grad=True)
    two = m.train_loss(*args, draws=draws, sampled=sampled, grad=True)
    torch.cuda.synchronize()
    for k in ("total", "parts", "num_pos", "grad"):
        assert torch.isfinite(one[k].float()).all() and torch.equal(one[k].view(torch.uint8), two[k].view(torch.uint8)), k
    assert torch.equal(one["example"]["labels"], ex["labels"])
    drawn = m.train_loss(*args, generator=torch.Generator(device=DEV).manual_seed(3), sampled=sampled)        # the same generator state: the same draws
    assert torch.equal(drawn["total"], one["total"])


def test_draw_follows_the_reference_distributions():
    from minddet_amd import det_ops

    aug = det_ops.PointCloudAugment((0, -39.68, 69.12, 39.68), gt_loc_noise_std=[0.25, 0.5, 1.0], gt_rotation_noise=[-0.157, 0.157], num_try=100)
    f = fixture_case("car")
    boxes = dev(np.stack([f["gt_boxes"], f["gt_boxes"][::-1]]))
    d = aug.draw(boxes, dev(np.array([12, 12], np.int32)), torch.Generator(device=DEV).manual_seed(1))
    loc, rot, grot, glob = (d[k].cpu().numpy() for k in ("loc", "rot", "grot", "glob"))
    assert loc.shape == (2, 12, 100, 3) and loc.dtype == rot.dtype == grot.dtype == glob.dtype == np.float64 and glob.shape == (2, 6)
    assert (rot >= -0.157).all() and (rot <= 0.157).all()
    shift = np.arctan2(boxes.cpu().numpy()[..., 0].astype(np.float64), boxes.cpu().numpy()[..., 1].astype(np.float64))[..., None]
    assert (grot >= 0.78 - shift - 1e-12).all() and (grot <= 2.35 - shift + 1e-12).all() and np.ptp(grot + shift) > 1.4
    assert set(glob[:, 0].tolist()) <= {0.0, 1.0} and (np.abs(glob[:, 1]) <= np.pi / 4).all() and (glob[:, 2] >= 0.95).all() and (glob[:, 2] <= 1.05).all()
    for k, std in enumerate((0.25, 0.5, 1.0)):             # per axis, 2 x 12 x 100 draws: the standard error of the std is 1.4 %
        assert abs(loc[..., k].std() / std - 1.0) <= 0.10, (k, loc[..., k].std())
    same = det_ops.PointCloudAugment((0, -39.68, 69.12, 39.68), gt_loc_noise_std=[0.25, 0.25, 0.25])
    one = same.draw(boxes[:1], None, torch.Generator(device=DEV).manual_seed(2))["loc"].cpu().numpy()
    assert one.size == 3600 and abs(one.std() / 0.25 - 1.0) <= 0.10, one.std()      # G x T x 3 = 3 600 draws: standard error 1.2 %
    flips = torch.stack([aug.draw(boxes, None, torch.Generator(device=DEV).manual_seed(k))["glob"][:, 0] for k in range(8)])
    assert 0 < float(flips.mean()) < 1
    off = det_ops.PointCloudAugment((0, -39.68, 69.12, 39.68), global_random_rot_range=[0, 0])
    assert off.draw(boxes, None)["grot"] is None and not off.enable_grot
