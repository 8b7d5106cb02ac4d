"""-m gpu: md_pp_loss / md_pp_loss_grad (det_ops.pp_loss, csrc/pploss.hip) against tests/pp_loss_contract.py, which the CPU tests show
equal to a literal transcription of the reference's loss under autograd.

Conditions, fixed beforehand: parts, num_pos and total within 1 fp32 ulp of the contract's float64 value rounded to fp32; grad exactly
+0.0 (the bits) on every structural zero -- padding channels, the cls channels of ignored anchors, the box / dir channels of
non-positive anchors -- and NaN nowhere; every other element within 1 ulp of the rounded contract value, with at most 1 in 10^4 of them
differing at all (device and numpy float64 exp / log / sin differ in the last bits only, so a differing element needs a value within
~2^-29 of an fp32 rounding tie; the cap is generous and the contract alone meets it); md_pp_loss bit-identical to md_pp_loss_grad in
parts / num_pos / total.  Then: the planted map, the settings, equal results across calls, streams and the scratch-pool form with
garbage-filled outputs, autograd through det_ops.point_pillars_loss, the two production shapes with targets from
det_ops.assign_targets_batch (its test too)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import pp_loss_contract as pl
from tests.conftest import has_gpu
from tests.test_pp_loss_cpu import FIXTURE_SHAPES, FURTHER, bf16, fixture, layout, predictions

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def attrs_of(lay, settings):
    from minddet_amd import det_ops

    s = dict(pl.DEFAULTS, **settings)
    return det_ops.pp_loss_attrs(dict(cls=lay["off_cls"], box=lay["off_box"], dir_cls=lay["off_dir"]), lay["num_anchors"], lay["num_classes"],
                                 s["alpha"], s["gamma"], s["sigma"], s["code_weights"], s["cls_weight"], s["loc_weight"], s["dir_weight"],
                                 s["pos_cls_weight"], s["neg_cls_weight"])


class Problem:
    """one call's inputs as numpy (head: the fp32 values of the bf16 outputs; pad: the channels no head owns, which get a bf16 NaN on the
    device) and the contract's result, computed once and shared read-only"""

    def __init__(self, head, labels, reg, anchors, lay, settings=None):
        self.head, self.labels, self.reg, self.anchors, self.lay, self.settings = head, labels, reg, anchors, lay, dict(settings or {})
        A, K = lay["num_anchors"], lay["num_classes"]
        used = set(range(lay["off_cls"], lay["off_cls"] + A * K)) | set(range(lay["off_box"], lay["off_box"] + A * 7))
        if lay["off_dir"] is not None:
            used |= set(range(lay["off_dir"], lay["off_dir"] + A * 2))
        self.pad = np.setdiff1d(np.arange(head.shape[3]), sorted(used))
        self.want = pl.loss(head, labels, reg, anchors, **lay, **dict(pl.DEFAULTS, **self.settings))
        for v in list(self.want.values()) + [head, labels, reg, anchors]:
            v.setflags(write=False)

    def device(self):
        h = torch.from_numpy(np.array(self.head))
        h[..., torch.from_numpy(self.pad)] = float("nan")                     # the pad channels never enter the arithmetic
        reg = np.array(self.reg)
        reg[self.labels <= 0] = np.nan                                        # nor do the targets of an anchor that is not positive
        dev = [torch.from_numpy(np.array(v)).to(DEV) for v in (self.labels, reg, self.anchors)]
        return [h.to(torch.bfloat16).to(DEV)] + dev, attrs_of(self.lay, self.settings)


def to_np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check(tag, got, want):
    """the conditions of the module docstring; prints the measured figures before it asserts"""
    worst = pl.compare_losses(got, want)
    n, ndiff, worst_g, wrong_zero, nans = pl.compare_grad(got["grad"], want)
    print(f"pp_loss[{tag}]: total {float(got['total'][0]):.6f}, parts {got['parts'].tolist()}, losses worst {worst} ulp; grad elements owed "
          f"{n}, differing {ndiff}, worst {worst_g} ulp, structural zeros that are not +0.0 {wrong_zero}, NaN {nans}")
    assert worst <= 1
    assert wrong_zero == 0 and nans == 0
    assert worst_g <= 1 and ndiff * 10000 <= n, (worst_g, ndiff, n)


def run(pr, grad=True, out=None):
    from minddet_amd import det_ops

    ops, at = pr.device()
    return det_ops.pp_loss(*ops, at, grad=grad, out=out)


@functools.lru_cache(maxsize=None)
def car_problem():
    """the `car` fixture as B = 2, H = 54, W = 62, A = 2, K = 1, C = 24 (3348 cells: 52 strips + 20): sample 1 is the same rows with its
    positives set to ignore, so a sample without a positive stands beside one with 16"""
    H, W, A, K = FIXTURE_SHAPES["car"]
    labels, reg, anchors = fixture("car")
    labels = np.concatenate([labels, np.where(labels > 0, -1, labels)]).astype(np.int32)
    reg = np.concatenate([reg, reg])
    lay, C_ = layout(A, K)
    assert C_ == 24
    pr = Problem(predictions(np.random.default_rng(1), (2, H, W, C_), lay), labels, reg, anchors, lay)
    assert pr.want["num_pos"].tolist() == [16.0, 0.0] and len(pr.pad) == 4
    return pr


@functools.lru_cache(maxsize=None)
def pedcyc_problem(tag=None):
    """the `pedcyc` fixture as B = 1, H = 40, W = 60, A = 4, K = 2, C = 48"""
    H, W, A, K = FIXTURE_SHAPES["pedcyc"]
    labels, reg, anchors = fixture("pedcyc")
    lay, C_ = layout(A, K)
    assert C_ == 48
    pr = Problem(predictions(np.random.default_rng(2), (1, H, W, C_), lay), labels, reg, anchors, lay, FURTHER.get(tag))
    assert pr.want["num_pos"].tolist() == [13.0] and {1, 2} <= set(np.unique(labels))
    return pr


@functools.lru_cache(maxsize=None)
def planted_problem():
    """B = 2 on a 3 x 5 map (15 cells: no multiple of the strip, and the second sample starts in the middle of what a strip would
    hold), A = 2, K = 3, heads in the order box, dir, cls in 32 channels (8 of padding): logits 0 and +-30, a label above K, pred equal
    to target, a direction sum of exactly 0, equal direction logits"""
    H, W, A, K = 3, 5, 2, 3
    N = H * W * A
    rng = np.random.default_rng(33)
    lay, C_ = layout(A, K, order=("box", "dir", "cls"), C=32)
    labels = np.zeros((2, N), np.int32)
    labels[0, [1, 4, 9, 17, 22, 29]] = [1, 2, 3, K + 2, 1, 3]
    labels[0, [2, 3, 11]] = -1
    labels[1, [0, 5, 28]] = -1
    labels[1, [7, 20]] = [2, 1]
    reg = bf16(rng.normal(0, 1, (2, N, 7)))
    anchors = np.zeros((N, 7), np.float32)
    anchors[:, 6] = np.tile([0.0, 1.57], N // 2)
    head = predictions(rng, (2, H, W, C_), lay)
    cells = head.reshape(2, H * W, C_)
    cls0 = lay["off_cls"]
    cells[0, 0, cls0:cls0 + 6] = [0.0, 30.0, -30.0, 30.0, 0.0, -30.0]         # anchor 0 background; anchor 1 label 1: its own class at +30
    cells[0, 2, cls0:cls0 + 6] = [-30.0, -30.0, 0.0, 30.0, -30.0, 0.0]        # anchor 4 label 2: own class at -30; anchor 5 background
    cells[0, 1, cls0:cls0 + 6] = [30.0, 0.0, -30.0, 0.0, 30.0, -30.0]         # anchors 2, 3: ignored
    cells[1, 3, cls0:cls0 + 6] = [0.0, 0.0, 0.0, 30.0, 30.0, 30.0]            # anchor 7 label 2
    n = 4                                                                     # pred equal to target on every code
    cells[0, n // A, lay["off_box"] + (n % A) * 7:lay["off_box"] + (n % A) * 7 + 7] = reg[0, n]
    n = 9                                                                     # reg + anchor rotation == 0 exactly: bin 0
    reg[0, n, 6] = -anchors[n, 6]
    n = 22                                                                    # equal direction logits
    cells[0, n // A, lay["off_dir"] + (n % A) * 2:lay["off_dir"] + (n % A) * 2 + 2] = 0.75
    pr = Problem(head, labels, reg, anchors, lay)
    assert pr.want["num_pos"].tolist() == [6.0, 2.0] and len(pr.pad) == 8 and (reg[0, 9, 6] + anchors[9, 6]) == 0
    return pr


@functools.lru_cache(maxsize=None)
def plain_problem():
    """no direction head, alpha None, gamma 0; 7 x 11 cells (two strips) of 19 channels: H W C is odd, the path without 16-byte accesses"""
    H, W, A, K = 7, 11, 2, 1
    N = H * W * A
    rng = np.random.default_rng(19)
    lay, C_ = layout(A, K, direction=False, C=19)
    labels = rng.choice(np.array([-1, 0, 0, 0, 1], np.int32), (3, N))
    labels[2] = np.where(labels[2] > 0, 0, labels[2])
    reg = rng.normal(0, 1, (3, N, 7)).astype(np.float32)
    anchors = rng.normal(0, 1, (N, 7)).astype(np.float32)
    pr = Problem(predictions(rng, (3, H, W, C_), lay), labels, reg, anchors, lay, dict(alpha=None, gamma=0.0))
    assert pr.want["num_pos"][2] == 0 and pr.want["num_pos"][0] > 10 and pr.want["parts"][2] == 0 and (H * W * C_) % 2 == 1
    return pr


@pytest.mark.parametrize("problem", [car_problem, pedcyc_problem, planted_problem, plain_problem], ids=["car", "pedcyc", "planted", "plain"])
def test_shape_equals_the_contract_and_forward_only_equals_forward_with_grad(problem):
    pr = problem()
    got = to_np(run(pr))
    check(problem.__name__, got, pr.want)
    fwd = to_np(run(pr, grad=False))
    assert set(fwd) == {"total", "parts", "num_pos"}
    for k in fwd:
        assert np.array_equal(bits(fwd[k]), bits(got[k])), k


def test_planted_values_land_where_the_header_says():
    pr = planted_problem()
    got = to_np(run(pr))
    lay, C_ = pr.lay, pr.head.shape[3]
    g = got["grad"].reshape(2, 15, C_)
    box, dr, cls = lay["off_box"], lay["off_dir"], lay["off_cls"]
    assert not g[0, 2, box:box + 7].any()                                     # pred equal to target
    d9 = g[0, 4, dr + 2:dr + 4]
    assert d9[0] < 0 < d9[1] and d9[0] == -d9[1]                              # a zero direction sum is bin 0
    d22 = g[0, 11, dr:dr + 2]
    assert abs(d22[1]) == abs(d22[0]) and pl.ulps_apart(abs(d22[0]), np.float32(pl.f32(0.2) / 2 * 0.5 / 6)) <= 1   # sigmoid(0) dir_weight / B / n_b
    row = g[0, 8, cls + 3:cls + 6]
    assert (row > 0).all() and g[0, 8, box + 7:box + 14].any()                # the label above K: a positive with an all-zero one-hot row
    assert bits(g[0, 1, cls:cls + 6]).tolist() == [0] * 6                     # ignored anchors, whatever their logits
    zero_logit = np.float32(1.0 / 2 * 0.75 / 6 * 0.25 * (2 * 0.5 * np.log(2.0) + 0.5))   # cls_weight / B (1 - alpha) / n_b m^2 (gamma (1 - m) ce + m)
    assert pl.ulps_apart(g[0, 0, cls], zero_logit) <= 1                       # a background logit of 0
    assert np.isnan(pr.device()[0][0].float().cpu().numpy()[..., pr.pad]).all()


@pytest.mark.parametrize("tag", ["gamma 1.5", "weights"])
def test_settings_equal_the_contract(tag):
    pr = pedcyc_problem(tag)
    check(tag, to_np(run(pr)), pr.want)


def test_equal_across_calls_streams_and_the_scratch_pool_with_garbage_filled_outputs():
    from minddet_amd import _lib, det_ops

    pr = car_problem()
    ops, at = pr.device()
    first = to_np(run(pr))

    def garbage():
        out = dict(total=torch.empty((1,), device=DEV), parts=torch.empty((5,), device=DEV), num_pos=torch.empty((2,), device=DEV),
                   grad=torch.empty(tuple(ops[0].shape), device=DEV))
        for v in out.values():
            v.view(torch.uint8).fill_(0xFF)
        return out

    filled = garbage()
    assert all(bool((v.view(torch.uint8) == 0xFF).all()) for v in filled.values())
    again = to_np(run(pr, out=filled))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs, pool, fwd = [garbage(), garbage()], [garbage(), garbage()], [garbage(), garbage()]
    torch.cuda.synchronize()
    for rep in range(2):                                                      # the second round reuses each stream's pool buffer
        for s, o, q, f in zip(streams, outs, pool, fwd):
            with torch.cuda.stream(s):
                det_ops.pp_loss(*ops, at, grad=True, out=o)
                assert _lib.call("md_pp_loss_grad", ops + [q["parts"], q["num_pos"], q["total"], q["grad"]], extra=at) == 0
                assert _lib.call("md_pp_loss", ops + [f["parts"], f["num_pos"], f["total"]], extra=at) == 0
    for o in [again] + [to_np(o) for o in outs + pool]:
        for k in ("total", "parts", "num_pos", "grad"):
            assert np.array_equal(bits(first[k]), bits(o[k])), k               # (a surviving 0xFF byte would differ from `first`)
    for f in fwd:
        f = to_np(f)
        for k in ("total", "parts", "num_pos"):
            assert np.array_equal(bits(first[k]), bits(f[k])), k
    check("car, again", first, pr.want)


def test_autograd_through_point_pillars_loss():
    from minddet_amd import det_ops

    pr = pedcyc_problem()
    (h, labels, reg, anchors), at = pr.device()
    lay = pr.lay
    loss = det_ops.PointPillarsLoss(dict(cls=lay["off_cls"], box=lay["off_box"], dir_cls=lay["off_dir"]), lay["num_anchors"], lay["num_classes"])
    assert bytes(loss.at) == bytes(at)
    ref = run(pr)
    x = h.clone().requires_grad_(True)
    total, parts, num_pos = det_ops.point_pillars_loss(x, labels, reg, anchors, loss)
    assert total.requires_grad and not parts.requires_grad and not num_pos.requires_grad
    up = torch.tensor([2.5], device=DEV)
    (g,) = torch.autograd.grad(total, x, grad_outputs=up)
    torch.cuda.synchronize()
    assert g.dtype == torch.bfloat16 and g.shape == x.shape
    assert torch.equal(total.detach(), ref["total"]) and torch.equal(parts, ref["parts"]) and torch.equal(num_pos, ref["num_pos"])
    want = (ref["grad"] * 2.5).to(torch.bfloat16)
    assert torch.equal(g.view(torch.int16), want.view(torch.int16)) and bool((g != 0).any())
    y = h.clone().requires_grad_(True)
    (det_ops.point_pillars_loss(y, labels, reg, anchors, loss)[0].sum() * 0.5).backward()
    assert torch.equal(y.grad.view(torch.int16), (ref["grad"] * 0.5).to(torch.bfloat16).view(torch.int16))


def seeded_ground_truth(rng, cfg, count):
    """`count` boxes (x, y, z, w, l, h, r) inside the config's range, sized as the anchors of a random class -> (boxes f32, classes i32)"""
    gens = cfg.model["anchor_generators"]
    x0, y0, _, x1, y1, _ = cfg.model["voxel_generator"]["point_cloud_range"]
    cls = rng.integers(1, cfg.model["num_class"] + 1, count).astype(np.int32)
    gt = np.zeros((count, 7), np.float32)
    gt[:, 0], gt[:, 1] = rng.uniform(x0 + 2, x1 - 2, count), rng.uniform(y0 + 2, y1 - 2, count)
    for i, c in enumerate(cls):
        g = gens[min(c - 1, len(gens) - 1)]
        gt[i, 2] = g["offsets"][2] + rng.uniform(-0.2, 0.2)
        gt[i, 3:6] = np.array(g["sizes"]) * rng.uniform(0.9, 1.1, 3)
    gt[:, 6] = rng.choice([0.0, 1.57, -1.57, 3.1], count) + rng.uniform(-0.2, 0.2, count)
    return gt, cls


@pytest.mark.parametrize("name,B,masked", [("car", 4, False), ("ped_cycle", 2, True)])
def test_production_shape_equals_the_contract_with_targets_from_the_batch_wrapper(name, B, masked):
    """the train config's shape: anchors from its generators, targets from det_ops.assign_targets_batch on seeded ground truth -- held
    to B single det_ops.assign_targets calls, bit for bit -- a seeded head tensor, and the loss through det_ops.PointPillarsLoss"""
    from minddet.models import Config
    from minddet_amd import det_ops

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", f"pointpillars_{name}_xyres16_train.py"))
    H, W = cfg.data["feature_map_hw"]
    gens = [det_ops.AnchorGeneratorStride(sizes=g["sizes"], anchor_strides=g["strides"], anchor_offsets=g["offsets"], rotations=g["rotations"],
                                          anchor_range=cfg.model["voxel_generator"]["point_cloud_range"]) for g in cfg.model["anchor_generators"]]
    A, K = sum(g.num_anchors_per_localization for g in gens), cfg.model["num_class"]
    anchors = det_ops.generate_anchors(gens, (1, H, W), device=DEV)["anchors"].reshape(-1, 7)
    N = H * W * A
    assert (name, H, W, N) in (("car", 248, 216, 107136), ("ped_cycle", 248, 296, 293632))
    rng = np.random.default_rng(248)
    gts = [seeded_ground_truth(rng, cfg, 12 + 3 * b) for b in range(B)]
    boxes, classes = [torch.from_numpy(g).to(DEV) for g, _ in gts], [torch.from_numpy(c).to(DEV) for _, c in gts]
    mask = torch.from_numpy((rng.uniform(size=(B, N)) < 0.7).astype(np.uint8)).to(DEV) if masked else None
    mt, ut = cfg.train_cfg["assigner"]["matched_threshold"], cfg.train_cfg["assigner"]["unmatched_threshold"]
    labels, reg, weights, gt_ids = det_ops.assign_targets_batch(anchors, boxes, classes, mt, ut, mask)
    assert labels.shape == (B, N) and labels.dtype == torch.int32 and reg.shape == (B, N, 7) and weights.shape == (B, N) and gt_ids.shape == (B, N)
    for b in range(B):
        one = det_ops.assign_targets(anchors, boxes[b], classes[b], mt, ut, None if mask is None else mask[b])
        for got, want in zip((labels, reg, weights, gt_ids), one):
            assert torch.equal(got[b].view(torch.int32), want.view(torch.int32))

    lay, C_ = layout(A, K)
    head = predictions(rng, (B, H, W, C_), lay)
    loss = det_ops.PointPillarsLoss(dict(cls=lay["off_cls"], box=lay["off_box"], dir_cls=lay["off_dir"]), A, K, cfg.train_cfg["loss"],
                                    cfg.train_cfg["direction_loss_weight"], cfg.train_cfg["pos_class_weight"], cfg.train_cfg["neg_class_weight"])
    hd = torch.from_numpy(head).to(torch.bfloat16).to(DEV)
    got = to_np(loss(hd, labels, reg, anchors, grad=True))
    want = pl.loss(head, labels.cpu().numpy(), reg.cpu().numpy(), anchors.cpu().numpy(), **lay, **pl.DEFAULTS)
    assert C_ == (24 if name == "car" else 48) and want["num_pos"].min() > 5 and (not masked or int((labels < 0).sum()) > N // 5)
    check(f"{name} b{B}", got, want)
    assert np.array_equal(bits(to_np(loss(hd, labels, reg, anchors))["total"]), bits(got["total"]))


def test_model_loss_runs_neck_head_and_loss():
    """graphs.PointPillarsKITTIPoints.loss / PointPillarsNet.loss on the tiny config: the front end, the neck and the head as forward()
    runs them, then the loss on that head tensor with the model's anchors; targets from the batch wrapper on the model's anchors"""
    from minddet_amd import det_ops, graphs
    from tests.test_pp_reader_gpu import _detector, small_cloud

    m = _detector("tiny_points")[0].to(DEV)
    assert type(m) is graphs.PointPillarsKITTIPoints and m.inner.train_cfg is None
    pts, offs = small_cloud(m, 2, 1500, 9)
    points, offsets = torch.from_numpy(pts).to(DEV), torch.from_numpy(offs).to(DEV)
    _, aux = m.forward(points, offsets, return_aux=True)
    anchors = m.inner.anchors
    rng = np.random.default_rng(4)
    boxes = []
    for b in range(2):                                                        # ground truth on top of a few anchors, slightly moved
        gt = anchors[torch.from_numpy(rng.choice(anchors.shape[0], 5, replace=False)).to(DEV)].clone()
        gt[:, :2] += 0.05
        boxes.append(gt)
    labels, reg, _, _ = det_ops.assign_targets_batch(anchors, boxes, None, 0.6, 0.45)
    example = dict(labels=labels, reg_targets=reg)
    out = m.loss(points, offsets, example, grad=True)
    assert torch.equal(out["head"].view(torch.int16), aux["head"].view(torch.int16))
    direct = det_ops.pp_loss(aux["head"], labels, reg, anchors, m.inner.loss_op().at, grad=True)
    inner = m.inner.loss(aux["pseudo_image"], example)
    torch.cuda.synchronize()
    for k in ("total", "parts", "num_pos", "grad"):
        assert torch.equal(out[k].view(torch.int32), direct[k].view(torch.int32)), k
    assert "grad" not in inner and torch.equal(inner["total"], direct["total"]) and float(out["num_pos"].min()) >= 5
    off = m.inner.head_offsets()
    hf = torch.nan_to_num(aux["head"].to(torch.float32)).cpu().numpy()
    want = pl.loss(hf, labels.cpu().numpy(), reg.cpu().numpy(), anchors.cpu().numpy(), off_cls=off["cls"], off_box=off["box"], off_dir=off["dir_cls"],
                   num_anchors=m.inner.num_anchors, num_classes=m.inner.num_class, **pl.DEFAULTS)
    check("tiny model", to_np({k: out[k] for k in ("total", "parts", "num_pos", "grad")}), want)
