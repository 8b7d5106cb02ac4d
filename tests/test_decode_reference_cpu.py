"""CPU checks of tests/decode_contract.py, the float64 decode references and data generators that tests/test_decode_production_gpu.py
holds the decode kernels to:

* every reference against the numpy oracle of the same op (oracle/nets.py yolo_decode_np, yolov8_decode_np, rcnn_candidates,
  rpn_level_decode; oracle/np_ops.py delta2bbox, centernet_decode, centerpoint_decode) on data away from the decision boundaries.  The
  oracles evaluate the ops' own fp32 operation sequences, so each of their continuous outputs must lie within the contract's bound of
  the float64 reference -- the same check the kernels face -- and every discrete output must match;
* each generator plants what its docstring claims;
* the references alone keep every case's either-outcome share under decode_contract.CAP, at the production calls' per-image shapes;
* oracle/nets.py::yolo_decode_np takes the class arg-max on the logits (saturated and underflowing classes)."""
import math

import numpy as np
import pytest
import torch

from oracle import nets, np_ops
from tests import decode_contract as dc

DEV = "cpu"
MR = abs(math.log(16 / 1000))
DEC_RPN = dict(means=[0.0] * 4, stds=[1.0] * 4, max_ratio=MR, clip_w=1344.0, clip_h=800.0)
DEC_RCNN = dict(means=[0.0] * 4, stds=[0.1, 0.1, 0.2, 0.2], max_ratio=MR, clip_w=1344.0, clip_h=800.0)
# CPU-sized calls with the production attributes (per-image shapes of the production calls; fewer images)
YOLO = ([4, 80, 80, 256], dict(num_classes=80, num_anchors=3, stride=8.0, anchors=[10.0, 13.0, 16.0, 30.0, 33.0, 23.0],
                                 conf_thres=0.25, out_offset=0, out_total=19200))
YOLO8 = ([2, 80, 80, 144], dict(num_classes=80, reg_max=16, stride=8.0, conf_thres=0.25, out_offset=0, out_total=6400))
RPN = ([[4, 50, 84, 16], [50 * 84 * 3, 4], [4, 1000], [4], [4, 1000, 4], [4, 1000]], dict(num_anchors=3, decode=DEC_RPN))
RCNN = dict(num_classes=80, reg_offset=88, score_thr=0.05, decode=DEC_RCNN)
HEAT = ([2, 128, 128, 88], dict(c0=0, num_classes=80, lo=1e-4, hi=1 - 1e-4))
CP_CFG = dict(score_threshold=0.1, out_size_factor=4, voxel_size=[0.2, 0.2], pc_range=[-51.2, -51.2],
              post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0])
CP_TASKS = [(dict(reg=0, height=2, dim=3, rot=6, vel=8, hm=10), 1), (dict(reg=11, height=13, dim=14, rot=17, vel=19, hm=21), 2)]


def cp_attrs(off, ncls):
    return dict(off_reg=off["reg"], off_height=off["height"], off_dim=off["dim"], off_rot=off["rot"], off_vel=off["vel"],
                off_hm=off["hm"], num_classes=ncls, score_threshold=CP_CFG["score_threshold"], out_size_factor=CP_CFG["out_size_factor"],
                voxel_size=CP_CFG["voxel_size"], pc_range=CP_CFG["pc_range"], post_center_range=CP_CFG["post_center_limit_range"])


def _ok(got, x, what):
    nb, worst, first = dc.check(got, x)
    assert nb == 0, f"{what}: {nb} elements off, first at {first}"
    assert worst <= 1.0
    return worst


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _fmax(a):
    """an oracle's -inf fill -> the kernels' -FLT_MAX"""
    return torch.where(torch.isinf(a) & (a < 0), torch.full_like(a, -dc.FLT_MAX), a)


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle's label rule (the md_yolo_decode fix)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_yolo_oracle_takes_arg_max_of_the_logits():
    """class logits 16 (class 0) and 17 (class 5): float32 sigmoids round both to 1.0 - 2^-24 / 1.0 ... and an arg-max after the
    sigmoid or on logits clamped to 16 picks class 0; every logit below -87: the sigmoids underflow alike.  The arg-max of the logits
    (first index on ties) gives 5, 3 and 1, and the score is obj * sigmoid(max logit)."""
    nc = 8
    h = np.zeros((1, 1, 3, 5 + nc), np.float32)
    h[..., 4] = 4.0
    h[0, 0, 0, 5:] = [16, 0, 0, 0, 0, 17, 0, 0]
    h[0, 0, 1, 5:] = [-100, -95, -110, -90, -120, -100, -100, -100]
    h[0, 0, 2, 5:] = [1, 3, 2, 3, 0, 0, 0, 0]
    _, s, lab = nets.yolo_decode_np(h, nc, 1, 8.0, [10.0, 13.0], 0.25)
    assert lab.tolist() == [[5, 3, 1]]
    sig = lambda v: 1.0 / (1.0 + np.exp(-np.float64(v)))
    np.testing.assert_array_equal(s[0], np.float32([np.float32(sig(4)) * np.float32(sig(17)), -np.inf,
                                                    np.float32(sig(4)) * np.float32(sig(3))]))


# ---------------------------------------------------------------------------------------------------------------------------------
# references against the oracles
# ---------------------------------------------------------------------------------------------------------------------------------
def test_yolo_reference_equals_oracle():
    shape, a = [2, 20, 20, 256], dict(YOLO[1], out_total=1200)
    (head,), _ = dc.gen_yolo(shape, a, 1, DEV)
    out, n, e = dc.yolo(head, a)
    bo, so, lo = nets.yolo_decode_np(head.float().numpy(), 80, 3, a["stride"], a["anchors"], a["conf_thres"])
    w = _ok(_f32(bo), out["boxes"], "boxes")
    _ok(_fmax(_f32(so)), out["scores"], "scores")
    _ok(torch.from_numpy(lo), out["labels"], "labels")
    assert e == 0 and w > 0


def test_yolov8_reference_equals_oracle():
    shape, a = [2, 20, 20, 144], dict(YOLO8[1], out_total=400)
    (head,), _ = dc.gen_yolov8(shape, a, 2, DEV)
    out, n, e = dc.yolov8(head, a)
    bo, so, lo = nets.yolov8_decode_np(head.float().numpy(), 80, 16, a["stride"], a["conf_thres"])
    _ok(_f32(bo), out["boxes"], "boxes")
    _ok(_fmax(_f32(so)), out["scores"], "scores")
    _ok(torch.from_numpy(lo), out["labels"], "labels")


def test_rcnn_scores_reference_equals_oracle():
    R, post, B = 400, 100, 4
    (cls_reg, cnt), _ = dc.gen_rcnn_scores([[R, 408], [B], [B, post * 80]], RCNN, 3, DEV)
    out, n, e = dc.rcnn_scores(cls_reg, cnt, RCNN, rows=(0, B, post))
    cand = nets.rcnn_candidates(cls_reg.float().numpy(), cnt.numpy(), 80, RCNN["score_thr"], post)
    _ok(_fmax(_f32(cand)).view(R, 80), out["cand"], "cand")
    assert e <= dc.CAP * n


def test_rpn_reference_equals_oracle():
    shapes = [[2, 25, 42, 16], [25 * 42 * 3, 4], [2, 300], [2], [2, 300, 4], [2, 300]]
    a = dict(num_anchors=3, decode=DEC_RPN)
    (head, anchors, idx, cnt), _ = dc.gen_rpn(shapes, a, 4, DEV)
    out, _, _ = dc.rpn_decode(head, anchors, idx, cnt, a)
    for b in range(2):
        c = int(cnt[b])
        bo, so = nets.rpn_level_decode(head[b].float().numpy(), anchors.numpy(), idx[b, :c].long().numpy(), 3, (800, 1344))
        ob, os_ = out["boxes"], out["scores"]
        _ok(_f32(bo), dc.Expect(val=ob.val[b, :c], want_val=ob.want_val[b, :c], want_fill=ob.want_fill[b, :c]), "boxes")
        _ok(_f32(so), dc.Expect(val=os_.val[b, :c], want_val=os_.want_val[b, :c], want_fill=os_.want_fill[b, :c]), "scores")


def test_rcnn_decode_reference_equals_delta2bbox():
    B, post, npre = 2, 200, 300
    (cls_reg, rois, sel, cnt), _ = dc.gen_rcnn_decode([[B * post, 408], [B * post, 5], [B, npre], [B], [B, npre, 4], [B, npre]], RCNN, 5,
                                                      DEV)
    out, _, _ = dc.rcnn_decode_selected(cls_reg, rois, sel, cnt, RCNN, post)
    for b in range(B):
        c = int(cnt[b])
        i = sel[b, :c].long()
        j, k = i // 80, i % 80
        r = b * post + j
        d = torch.stack([cls_reg[r, 88 + k * 4 + t] for t in range(4)], -1).float().numpy()
        bo = np_ops.delta2bbox(rois[r, 1:].numpy(), d, stds=(0.1, 0.1, 0.2, 0.2), max_shape=(800, 1344))
        ob = out["boxes"]
        _ok(_f32(bo), dc.Expect(val=ob.val[b, :c], want_val=ob.want_val[b, :c], want_fill=ob.want_fill[b, :c]), "boxes")


def test_heat_peaks_and_assemble_reference_equal_centernet_decode():
    shape, a = [2, 40, 136, 88], HEAT[1]
    (head,), _ = dc.gen_heat(shape, a, 6, DEV)
    hm_t, heat, peak, n, e = dc.heat_peaks(head, a)
    hm32 = np_ops.sigmoid_clip(head[..., :80].float().numpy().transpose(0, 3, 1, 2))
    _ok(_f32(hm32), dc.Expect(val=hm_t, want_val=torch.ones(hm_t.v.shape, dtype=torch.bool),
                             want_fill=torch.zeros(hm_t.v.shape, dtype=torch.bool)), "hm")
    wh = torch.rand((2, 2, 40, 136), dtype=torch.float32) * 30
    reg = torch.rand((2, 2, 40, 136), dtype=torch.float32)
    K = 100
    det, inds, cls = np_ops.centernet_decode(hm32, wh.numpy(), reg.numpy(), K)
    pad = np.full((2, 80, 42, 138), -np.inf, np.float32)
    pad[:, :, 1:-1, 1:-1] = hm32
    hmax = hm32.copy()
    for dy in range(3):
        for dx in range(3):
            hmax = np.maximum(hmax, pad[:, :, dy:dy + 40, dx:dx + 136])
    oheat = hm32 * (hm32 == hmax)
    _ok(_f32(oheat), heat, "heat")
    flat = oheat.reshape(2, 80, -1)
    order = np.argsort(-flat, axis=2, kind="stable")[:, :, :K]
    flat2 = np.take_along_axis(flat, order, 2).reshape(2, -1)
    order2 = np.argsort(-flat2, axis=1, kind="stable")[:, :K]
    ts = np.take_along_axis(flat2, order2, 1)
    x, _, _ = dc.centernet_assemble(_f32(ts), torch.from_numpy(order2.astype(np.int32)), torch.from_numpy(order.astype(np.int32)), wh, reg)
    _ok(_f32(det), x["det"], "det")
    _ok(torch.from_numpy(inds), x["inds"], "inds")
    _ok(torch.from_numpy(cls), x["cls"], "cls")


@pytest.mark.parametrize("task", range(len(CP_TASKS)))
def test_centerpoint_reference_equals_oracle(task):
    off, ncls = CP_TASKS[task]
    a = cp_attrs(off, ncls)
    (head,), _ = dc.gen_centerpoint([2, 128, 128, 72], a, 7 + task, DEV)
    out, n, e = dc.centerpoint(head, a)
    s, lab, bx, nb, _ = np_ops.centerpoint_decode(head.float().numpy(), off, ncls, CP_CFG)
    _ok(_f32(s), out["scores"], "scores")
    _ok(torch.from_numpy(lab), out["labels"], "labels")
    _ok(_f32(bx), out["boxes"], "boxes")
    _ok(_f32(nb), out["nms_boxes"], "nms_boxes")
    assert e <= dc.CAP * n


# ---------------------------------------------------------------------------------------------------------------------------------
# the generators plant what they claim
# ---------------------------------------------------------------------------------------------------------------------------------
def _has_every_finite_bf16(t):
    bits = t.reshape(-1).contiguous().view(torch.int16).long() & 0xFFFF
    seen = torch.zeros(65536, dtype=torch.bool)
    seen[bits] = True
    return int(seen.sum()) >= dc.N_BF16_FINITE and bool(seen[dc.all_finite_bf16().view(torch.int16).long() & 0xFFFF].all())


def _check_class_plants(cls, plants):
    for kind in ("tie", "sat", "low"):
        rows, want = plants[kind]
        assert rows.numel() > 0
        x = cls[rows].float()
        assert torch.equal(x.argmax(-1), want), kind
        if kind == "tie":
            assert bool(((x == x.max(-1, keepdim=True).values).sum(-1) == 2).all())
        elif kind == "sat":
            assert bool((x.max(-1).values == 17).all()) and bool(((x == 16).sum(-1) >= 1).all())
            assert bool(((x == 16).float().argmax(-1) < want).all())
        else:
            assert bool((x < -87).all()) and bool((want >= 1).all())


def test_yolo_generator_plants():
    shape, a = YOLO
    (head,), p = dc.gen_yolo(shape, a, 11, DEV)
    assert bool(torch.isnan(head[..., 255:].float()).all()) and not bool(torch.isnan(head[..., :255].float()).any())
    rows = head[..., :255].reshape(-1, 85)
    _check_class_plants(rows[:, 5:], p)
    assert p["obj"] is not None and _has_every_finite_bf16(rows[:, 4])
    (head8,), p8 = dc.gen_yolov8(*YOLO8, 12, DEV)
    _check_class_plants(head8.reshape(-1, 144)[:, 64:], p8)


def test_rpn_generator_plants():
    shapes, a = RPN
    (head, anchors, idx, cnt), p = dc.gen_rpn(shapes, a, 13, DEV)
    n = anchors.shape[0]
    assert cnt.tolist() == [0, 333, 1000, 999]
    for b in range(4):
        assert idx[b].unique().numel() == 1000 and {0, n - 1} <= set(idx[b].tolist())
    assert bool(torch.isnan(head[..., 15].float()).all()) and not bool(torch.isnan(head[..., :15].float()).any())
    # boxes across every image edge
    assert bool((anchors[:, 0] < 0).any()) and bool((anchors[:, 1] < 0).any()) and bool((anchors[:, 2] > 1344).any()) and \
        bool((anchors[:, 3] > 800).any())
    # the selected logits run through consecutive finite bf16 values
    allv = dc.all_finite_bf16()
    hf = head.view(4, -1, 16)
    live = torch.arange(1000)[None] < cnt[:, None]
    bi, ji = live.nonzero(as_tuple=True)
    ids = idx[bi, ji].long()
    got = hf[bi, ids // 3, ids % 3].view(torch.int16)
    want = allv[(p["offset"] + torch.arange(bi.numel())) % dc.N_BF16_FINITE].view(torch.int16)
    assert torch.equal(got, want)
    for (bb, jj), sgn in zip(p["big"], (1.0, -1.0)):
        assert bb.numel() > 0
        i2 = idx[bb, jj].long()
        dw = hf[bb, i2 // 3, 3 + (i2 % 3) * 4 + 2].float()
        dh = hf[bb, i2 // 3, 3 + (i2 % 3) * 4 + 3].float()
        assert bool((dw == 8 * sgn).all()) and bool((dh == -8 * sgn).all()) and 8 > MR


def test_rcnn_generator_plants():
    B, post, npre = 4, 1000, 2048
    (cls_reg, cnt), _ = dc.gen_rcnn_scores([[B * post, 408], [B], [B, post * 80]], RCNN, 14, DEV)
    assert cnt.tolist() == [0, 333, 1000, 999]
    assert bool(torch.isnan(cls_reg[:, 81:].float()).all()) and not bool(torch.isnan(cls_reg[:, :81].float()).any())
    (x, rois, sel, sc), _ = dc.gen_rcnn_decode([[B * post, 408], [B * post, 5], [B, npre], [B], [B, npre, 4], [B, npre]], RCNN, 15, DEV)
    assert sc.tolist() == [0, 682, 2048, 2047]
    for b in range(B):
        assert sel[b].unique().numel() == npre and {0, post * 80 - 1} <= set(sel[b].tolist())
    assert bool(torch.isnan(x[:, :88].float()).all()) and not bool(torch.isnan(x[:, 88:].float()).any())
    d = x[:, 88:].float().view(-1, 80, 4)
    assert bool((d[:, 3, 2] * 0.2 > MR).all()) and bool((d[:, 5, 3] * 0.2 > MR).all())
    assert bool((rois[:, 3] > rois[:, 1]).all()) and bool((rois[:, 4] > rois[:, 2]).all())
    assert torch.equal(rois[:, 0], (torch.arange(B * post) // post).float())


def test_mask_generator_plants():
    R, S, nc = 200, 28, 80
    (logits, dets), p = dc.gen_mask([[R, S, S, nc], [R, 6], [R, S, S]], nc, 16, DEV)
    r = torch.arange(R)
    assert bool((dets[r % 10 == 1, 4] == 0).all()) and bool((dets[r % 10 == 3, 4] < 0).all())
    assert bool((dets[r % 10 == 5, 5] == -1).all()) and bool((dets[r % 10 == 7, 5] == nc).all())
    v = p["valid"]
    assert torch.equal(v, (dets[:, 4] > 0) & (dets[:, 5] >= 0) & (dets[:, 5] < nc))
    lab = dets[:, 5].long().clamp(0, nc - 1)
    own = torch.gather(logits.view(R, S * S, nc), 2, lab.view(R, 1, 1).expand(R, S * S, 1))[..., 0]
    assert not bool(torch.isnan(own[v].float()).any()) and bool(torch.isnan(own[~v].float()).all())
    assert int((~torch.isnan(logits.float())).sum()) == int(v.sum()) * S * S       # every other channel NaN
    assert p["all_bf16"] and _has_every_finite_bf16(own[v])


def test_heat_generator_plants():
    shape, a = HEAT
    (head,), p = dc.gen_heat(shape, a, 17, DEV)
    assert bool(torch.isnan(head[..., 80:].float()).all()) and p["all_bf16"] and _has_every_finite_bf16(head[..., :80])
    names = {n for _, _, n, _, _ in p["planted"]}
    assert names == {"seam", "seam_clip_hi", "seam_clip_lo", "seam_higher", "corner", "far_corner"}
    hm, heat, peak, _, _ = dc.heat_peaks(head, a)
    hi, lo = dc.f32(a["hi"]), dc.f32(a["lo"])
    for b, c, name, cells, want in p["planted"]:
        ys, xs = [y for y, _ in cells], [x for _, x in cells]
        assert torch.equal(peak[b, c, ys, xs], torch.tensor(want)), name
        if name == "seam_clip_hi":
            assert bool((hm.v[b, c, ys, xs] == hi).all()) and bool((hm.e[b, c, ys, xs] == 0).all())
            assert len(set(head[b, ys, xs, c].float().tolist())) == 4
        if name == "seam_clip_lo":
            assert bool((hm.v[b, c, ys, xs] == lo).all()) and bool((hm.e[b, c, ys, xs] == 0).all())
        if name.startswith("seam"):
            assert any((y + 1) % 8 == 0 and y + 1 in ys for y in ys)
            assert {63, 64} <= set(xs)
        if name == "corner":
            assert (0, 0) in cells
        if name == "far_corner":
            assert (127, 127) in cells


def test_centerpoint_generator_plants():
    off, ncls = CP_TASKS[1]
    a = cp_attrs(off, ncls)
    B, H, W, C = 4, 128, 128, 72
    (head,), p = dc.gen_centerpoint([B, H, W, C], a, 18, DEV)
    f = head.view(-1, C).float()
    own = set(range(off["reg"], off["hm"] + ncls))
    other = [c for c in range(C) if c not in own]
    assert bool(torch.isnan(f[:, other]).all()) and not bool(torch.isnan(f[:, sorted(own)]).any())
    assert p["all_bf16"] and _has_every_finite_bf16(f[:, off["hm"]:off["hm"] + ncls].to(torch.bfloat16))
    r = torch.arange(f.shape[0])
    edge = torch.zeros_like(r, dtype=torch.bool)
    for e in p["edges"]:
        edge[e] = True
    m = lambda k: (r % dc.CP_MOD == k) & ~edge
    hm = f[:, off["hm"]:off["hm"] + ncls]
    assert bool((hm[m(5)] == 1.0).all()) and bool((hm[m(9)] >= 17).all())
    assert bool((f[m(13), off["rot"]:off["rot"] + 2] == 0).all())
    assert bool((f[m(17), off["height"]] == 10).all()) and bool((f[m(19), off["height"]] == -10).all())
    assert bool((f[m(23), off["height"]] == 10.0625).all())
    out, n, e = dc.centerpoint(head, a)
    xs = (r % (H * W) % W).double() + f[:, off["reg"]].double()
    ys = (r % (H * W) // W).double() + f[:, off["reg"] + 1].double()
    for rows, v, lim in zip(p["edges"], (xs, xs, ys, ys), (61.2, -61.2, 61.2, -61.2)):
        assert rows.numel() == B
        c = v[rows] * 4 * dc.f32(0.2) + dc.f32(-51.2)
        assert bool(((c - lim).abs() < 1e-5).all())
    # the edge cells are the either-outcome decisions; rot (0, 0) cells decode to rot 0
    assert 0 < e <= dc.CAP * n
    ok = out["scores"].want_fill.view(-1) == 0
    rot0 = m(13) & ok
    assert bool((out["boxes"].val.v.view(-1, 9)[rot0, 8] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# the references alone keep every case under the cap
# ---------------------------------------------------------------------------------------------------------------------------------
def _share(n, e):
    print(f"either-outcome {e} of {n} ({100 * e / max(n, 1):.4f} %)")
    return e / max(n, 1)


def test_either_outcome_share_under_cap():
    shape, a = YOLO
    (head,), _ = dc.gen_yolo(shape, a, 21, DEV)
    assert _share(*dc.yolo(head, a)[1:]) <= dc.CAP
    (head,), _ = dc.gen_yolov8(*YOLO8, 22, DEV)
    assert _share(*dc.yolov8(head, YOLO8[1])[1:]) <= dc.CAP
    B, post = 4, 1000
    (cls_reg, cnt), _ = dc.gen_rcnn_scores([[B * post, 408], [B], [B, post * 80]], RCNN, 23, DEV)
    assert _share(*dc.rcnn_scores(cls_reg, cnt, RCNN, rows=(0, B, post))[1:]) <= dc.CAP
    (head,), _ = dc.gen_heat(*HEAT, 24, DEV)
    _, _, _, n, e = dc.heat_peaks(head, HEAT[1])
    assert _share(n, e) <= dc.CAP
    for t, (off, ncls) in enumerate(CP_TASKS):
        a = cp_attrs(off, ncls)
        (head,), _ = dc.gen_centerpoint([4, 128, 128, 72], a, 25 + t, DEV)
        assert _share(*dc.centerpoint(head, a)[1:]) <= dc.CAP
