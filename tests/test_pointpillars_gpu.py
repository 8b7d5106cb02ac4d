"""-m gpu: the anchor-based (KITTI) PointPillars on the device -- md_pp_scores and md_pp_decode_selected against the float64 contract
of tests/pp_contract.py and, bit for bit, against the stand-alone operators they fuse; the five-launch chain stage by stage from the
device's own tensors; the merged 1x1 heads against three separate launches and against float64; the detector end to end."""
import math

import numpy as np
import pytest
import torch

from tests import conv_contract as cc
from tests import neck_checks
from tests import pp_contract as ppc
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
NMS = dict(nms_pre_max_size=900, nms_post_max_size=300, nms_score_threshold=0.09, nms_iou_threshold=0.01)
PI32 = torch.tensor(math.pi, dtype=torch.float32)
_cache = {}


def case(name):
    """head, attributes, anchors, mask (sample 0 entirely masked) and the device chain's tensors of one shape: made once"""
    if name not in _cache:
        from minddet_amd import det_ops

        head, a, plants = ppc.make_head(name, device=DEV)
        anchors, mask = ppc.make_anchors(name, DEV), ppc.make_mask(name, device=DEV, all_masked_sample=0)
        post = det_ops.PPHeadPost(dict(a, **NMS))
        out, aux = post(head, anchors, mask, return_aux=True)
        torch.cuda.synchronize()
        _cache[name] = dict(head=head, a=a, plants=plants, anchors=anchors, mask=mask, post=post, out=out, aux=aux)
    return _cache[name]


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return bool((bits(a) == bits(b)).all())


# ------------------------------------------------------------------------------------------------------------------- 1. md_pp_scores
@pytest.mark.parametrize("name", list(ppc.SHAPES))
def test_scores_against_the_contract(name):
    from minddet_amd import det_ops

    c = case(name)
    B, H, W, A, K, C = ppc.SHAPES[name]
    for mask in ((c["mask"], None) if name in ("clamp", "odd") else (c["mask"],)):
        if mask is None:
            sc, lab = det_ops.pp_scores(c["head"], c["a"]["off_cls"], A, K, None)
        else:
            sc, lab = c["aux"]["scores"], c["aux"]["labels"]
        want, n_dec, n_either = ppc.scores(c["head"], mask, c["a"])
        nb, worst, first = ppc.check(sc, want["scores"])
        print(f"{name} mask={mask is not None}: scores worst err / bound {worst:.3f}, either {n_either} of {n_dec}")
        assert nb == 0 and worst <= 1.0, (name, nb, worst, first)
        assert n_either <= ppc.CAP * n_dec
        if mask is not None:
            assert bool((bits(sc)[mask == 0] == bits(torch.tensor([-1.0]))[0].item()).all()) and bool((sc[mask != 0] >= 0).all())
            assert bool((sc[0] == -1).all())                                  # the all-masked sample
        else:
            assert bool((sc >= 0).all())
        assert bool(want["labels"](lab).all()) and bool(((lab >= 0) & (lab < K)).all())
        if K > 1:
            for b in range(B):                                                # exact logit ties go to the lower class; labels of masked anchors too
                t = c["plants"]["ties"][b].to(DEV)
                assert bool((lab[b, t] == 0).all())
                s = c["plants"]["saturated"][b].to(DEV)
                assert bool((lab[b, s] == 0).all()) and (mask is not None or bool((sc[b, s] == 1.0).all()))


# ---------------------------------------------------------------------------------------------------------- 2. md_pp_decode_selected
@pytest.mark.parametrize("name", list(ppc.SHAPES))
def test_decode_selected_on_the_devices_own_topk(name):
    from minddet_amd import det_ops

    c = case(name)
    B, H, W, A, K, C = ppc.SHAPES[name]
    N, a, aux = H * W * A, c["a"], c["aux"]
    idx, cnt, vals = aux["topk_idx"], aux["topk_cnt"], aux["topk_values"]
    k = idx.shape[1]
    assert k == min(900, N) and aux["selected"].shape == (B, k, 9)
    live = torch.arange(k, device=DEV)[None] < cnt[:, None]
    assert int(cnt[0]) == 0 and bool(live[1:].any())
    ii = torch.where(live, idx.long(), torch.zeros_like(idx.long()))
    # every anchor through the stand-alone operator, gathered at idx: bit-identical boxes
    enc = c["head"][..., a["off_box"]:a["off_box"] + 7 * A].float().reshape(B, N, 7)
    dec_all = det_ops.second_box_decode(enc, c["anchors"])
    want_box = torch.where(live[..., None], torch.gather(dec_all, 1, ii[..., None].expand(B, k, 7)), torch.zeros((), device=DEV))
    assert same_bits(aux["boxes"], want_box)
    assert same_bits(aux["standup"], det_ops.standup_boxes(want_box.reshape(-1, 7)).reshape(B, k, 4))
    dl = c["head"][..., a["off_dir"]:a["off_dir"] + 2 * A].float().reshape(B, N, 2)
    dirs = (torch.gather(dl[..., 1], 1, ii) > torch.gather(dl[..., 0], 1, ii)).to(torch.int32) * live
    assert bool((aux["dir_labels"] == dirs).all())
    for b in range(B):                                                           # a direction tie goes to bin 0
        t = c["plants"]["dir_ties"][b].to(DEV)
        hit = live[b] & torch.isin(idx[b].long(), t)
        assert bool((aux["dir_labels"][b][hit] == 0).all())
    sel = aux["selected"]
    rot = want_box[..., 6]
    fix = ((rot > 0) != (dirs != 0)) & live
    assert bool(fix.any()) and bool((~fix & live).any())
    assert same_bits(sel[..., :6], want_box[..., :6]) and same_bits(sel[..., 6], torch.where(fix, rot + PI32.to(DEV), rot))
    assert same_bits(sel[..., 7], torch.where(live, vals, torch.zeros_like(vals))) and bool((vals[live] >= np.float32(0.09)).all())
    assert bool((sel[..., 8] == torch.gather(aux["labels"], 1, ii).float() * live).all())
    for t in (sel, aux["standup"], aux["boxes"], aux["dir_labels"]):
        assert not bool(t[~live].any())                                          # rows >= cnt are all zero
    # and the values against float64
    want, n_dec, n_either = ppc.decode_selected(c["head"], c["anchors"], idx, cnt, vals, aux["labels"], a)
    assert n_either <= ppc.CAP * max(n_dec, 1)
    for key, got in (("boxes", aux["boxes"]), ("standup", aux["standup"])):
        nb, worst, first = ppc.check(got, want[key])
        print(f"{name}: {key} worst err / bound {worst:.3f}")
        assert nb == 0 and worst <= 1.0, (name, key, nb, worst, first)
    assert bool(want["rot"](sel[..., 6]).all()) and bool((aux["dir_labels"].long() == want["dir_labels"]).all())


def test_decode_selected_skips_indices_outside_the_anchor_table():
    from minddet_amd import det_ops

    c = case("clamp")
    B, H, W, A, K, C = ppc.SHAPES["clamp"]
    N = H * W * A
    idx = torch.tensor([[0, -1, N, N - 1, 2 ** 31 - 1], [5, 6, 7, 8, 9]], dtype=torch.int32, device=DEV)
    cnt = torch.tensor([5, 9], dtype=torch.int32, device=DEV)                    # a count beyond k is clamped
    vals = torch.full((2, 5), 0.5, device=DEV)
    labels = torch.zeros((B, N), dtype=torch.int32, device=DEV)
    dets, st, dirs, boxes = det_ops.pp_decode_selected(c["head"], c["anchors"], idx, cnt, vals, labels, c["a"]["off_box"], c["a"]["off_dir"], A,
                                                       with_boxes=True)
    bad = torch.tensor([[False, True, True, False, True], [False] * 5], device=DEV)
    for t in (dets, st, boxes, dirs):
        assert not bool(t[bad].any())
    assert bool((dets[~bad][:, 3:6] > 0).all()) and bool((dets[~bad][:, 7] == 0.5).all())
    # no direction classifier: no fix, bins 0
    d2, _, dr2 = det_ops.pp_decode_selected(c["head"], c["anchors"], idx, cnt, vals, labels, c["a"]["off_box"], None, A)
    assert same_bits(d2[..., 6], boxes[..., 6]) and not bool(dr2.any())


# ---------------------------------------------------------------------------------------------------------------------- 3. the chain
@pytest.mark.parametrize("name", list(ppc.SHAPES))
def test_chain_stage_by_stage_from_device_tensors(name):
    import oracle
    from minddet_amd import det_ops

    c = case(name)
    B, H, W, A, K, C = ppc.SHAPES[name]
    N, a, aux = H * W * A, c["a"], c["aux"]
    dets, count = c["out"]
    k, post = min(900, N), NMS["nms_post_max_size"]
    assert dets.shape == (B, post, 9) and count.shape == (B,) and count.dtype == torch.int32
    if name == "ped_cycle":                                        # this shape reaches the top-k's multi-workgroup form
        det_ops.topk_segmented(aux["scores"], torch.arange(0, (B + 1) * N, N, dtype=torch.int32, device=DEV), k, max_segment=N)
        assert det_ops._lib.lib().md_topk_last_path() == 3
    # top-k == a stable descending sort of the device's own scores, threshold as >=
    sv, si = torch.sort(aux["scores"], dim=1, descending=True, stable=True)
    cnt = torch.minimum((aux["scores"] >= np.float32(NMS["nms_score_threshold"])).sum(1), torch.tensor(k, device=DEV)).to(torch.int32)
    assert bool((aux["topk_cnt"] == cnt).all())
    live = torch.arange(k, device=DEV)[None] < cnt[:, None]
    assert bool((aux["topk_idx"].long() == si[:, :k])[live].all()) and same_bits(torch.where(live, aux["topk_values"], sv[:, :k]), sv[:, :k])
    # NMS keep list against the oracle on the device's own standup boxes
    st, kidx, cn = aux["standup"].cpu().numpy(), aux["keep_idx"].cpu().numpy(), count.cpu().numpy()
    for b in range(B):
        n = int(cnt[b])
        keep = np.nonzero(oracle.nms_aligned(st[b, :n], NMS["nms_iou_threshold"], 0.0, mode=0))[0][:post]
        assert cn[b] == len(keep), (b, cn[b], len(keep))
        np.testing.assert_array_equal(kidx[b, :len(keep)], keep)
    assert cn[0] == 0 and not bool(dets[0].any())                  # no score passes the threshold: count 0, zero rows
    assert cn[1:].min() > 0
    # final rows: the per-sample composition of the stand-alone operators on the same head tensor
    cls = det_ops.sigmoid_clip(c["head"][..., :A * K].float().reshape(B, N, K), 0.0, 1.0)        # 1 / (1 + expf(-x)), the clip idle
    enc = c["head"][..., a["off_box"]:a["off_box"] + 7 * A].float().reshape(B, N, 7)
    dec_all = det_ops.second_box_decode(enc, c["anchors"])
    dl = c["head"][..., a["off_dir"]:a["off_dir"] + 2 * A].float().reshape(B, N, 2)
    dir_all = dl[..., 1] > dl[..., 0]
    for b in range(B):
        boxes, scores, labels, n = det_ops.pp_get_selected_data(cls[b], dec_all[b], c["mask"][b].bool(), NMS)
        n = int(n)
        assert n == cn[b]
        anchor = torch.gather(aux["topk_idx"][b].long(), 0, aux["keep_idx"][b, :n].long())          # verified above
        rot = boxes[:n, 6]
        fixed = torch.where((rot > 0) != dir_all[b][anchor], rot + PI32.to(DEV), rot)
        want = torch.cat([boxes[:n, :6], fixed[:, None], scores[:n, None], labels[:n, None].float()], 1)
        assert same_bits(dets[b, :n], want), b
        assert not bool(dets[b, n:].any())
        assert bool((dets[b, :n, 7][:-1] >= dets[b, :n, 7][1:]).all())


# ---------------------------------------------------------------------------------------------------------------------- 4. the heads
@pytest.mark.parametrize("A,K", [(2, 1), (4, 2)])
def test_merged_heads_equal_three_launches_and_float64(A, K):
    from minddet_amd import graphs, nn_ops

    head = graphs.PPAnchorHead(graphs.ParamInit(3), 384, A, K).to(DEV)
    g = torch.Generator().manual_seed(5)
    x = (torch.randn((2, 31, 33, 384), generator=g) * 0.7).clamp(min=0).to(torch.bfloat16).to(DEV)      # post-ReLU features
    y = head(x)
    total = A * K + A * 7 + A * 2
    assert y.shape == (2, 31, 33, (total + 7) // 8 * 8)
    off = head.head_offsets()
    for m, o in zip(head.children(), (off["cls"], off["box"], off["dir_cls"])):
        alone = m(x)
        assert torch.equal(alone[..., :m.cout].view(torch.int16), y[..., o:o + m.cout].view(torch.int16)), o
        wl = m.weight.to(torch.bfloat16).double().permute(0, 2, 3, 1).to(DEV)                        # the packed operand's values
        want, bound = cc.conv_stage(x.double(), 0.0, wl, m.bias.to(DEV), cc._plain(2, 31, 33, 384, 1, 1, 0, m.cout), 0)
        err = (alone[..., :m.cout].double() - want).abs()
        print(f"A={A} K={K} cout={m.cout}: worst err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())


# -------------------------------------------------------------------------------------------------------------------- 5. the detector
def _detector(name, seed=7, **over):
    from tests.test_pointpillars_cpu import _detector as build

    m, cfg = build(name, seed, **over)
    return m.to(DEV), cfg


def _pseudo(B, hw, seed, fill=0.15):
    """a sparse pseudo-image: about `fill` of the cells hold a pillar's non-negative features"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, hw[0], hw[1], 64), generator=g) * 1.5
    occ = torch.rand((B, hw[0], hw[1], 1), generator=g) < fill
    return (x * occ).to(torch.bfloat16).to(DEV), occ[..., 0]


def _structure(dets, count, post, thr, K):
    d, c = dets.cpu(), count.cpu()
    assert d.shape[1:] == (post, 9) and c.dtype == torch.int32
    for b in range(d.shape[0]):
        n = int(c[b])
        assert 0 <= n <= post and not bool(d[b, n:].any())
        assert bool((d[b, :n, 7][:-1] >= d[b, :n, 7][1:]).all()) and bool((d[b, :n, 7] >= np.float32(thr)).all())
        assert bool(((d[b, :n, 8] >= 0) & (d[b, :n, 8] < K) & (d[b, :n, 8] == d[b, :n, 8].round())).all())
        assert bool((d[b, :n, 3:6] > 0).all()) and bool(torch.isfinite(d[b, :n]).all())


def test_tiny_detector_end_to_end():
    from minddet_amd import det_ops, weights

    m, cfg = _detector("tiny")
    x, occ = _pseudo(4, m.grid_hw, 11)
    # the anchors mask from voxel coordinates, against det_ops.anchors_mask per sample
    coors, nums = [], []
    for b in range(4):
        yx = occ[b].nonzero()
        cb = torch.cat([torch.full((yx.shape[0], 1), b), torch.zeros((yx.shape[0], 1), dtype=torch.long), yx], 1).to(torch.int32)
        nums.append(cb.shape[0])
        coors.append(torch.cat([cb, torch.full((600 - cb.shape[0], 4), 7, dtype=torch.int32)]))            # rows past voxel_num: ignored
    coors, voxel_num = torch.stack(coors).to(DEV), torch.tensor(nums, dtype=torch.int32, device=DEV)
    mask = m.anchors_mask_from_coors(coors, voxel_num)
    N = m.anchors.shape[0]
    assert mask.shape == (4, N) and mask.dtype == torch.uint8 and 0 < int(mask.sum()) < mask.numel()
    for b in range(4):
        _, mb = det_ops.anchors_mask(coors[b, :nums[b], 1:].contiguous(), (m.grid_hw[1], m.grid_hw[0]), m.anchors_bv, m.voxel_size, m.pc_range, 1)
        assert torch.equal(mask[b].bool(), mb)
    post, thr = cfg.test_cfg["nms_post_max_size"], cfg.test_cfg["nms_score_threshold"]
    plain = m.forward(x[:3])
    masked, aux = m.forward(x[:3], anchors_mask=mask[:3], return_aux=True)
    for dets, count in (plain, masked):
        _structure(dets, count, post, thr, 2)
        assert int(count.min()) > 0
    assert aux["head"].shape == (3, 16, 24, 48) and aux["neck"].shape == (3, 16, 24, 48)
    assert bool((aux["scores"][mask[:3] == 0] == -1).all()) and not torch.equal(plain[0], masked[0])
    # two streams are bit-identical to one (the mask is split with the batch)
    m2, _ = _detector("tiny")
    from minddet_amd import graphs
    graphs._split_forward_of(m2, dict(streams=2))
    for mk in (None, mask):
        one = m.forward(x, anchors_mask=mk)
        two = m2.forward_streams(x, mk)
        torch.cuda.synchronize()
        assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    # reload through the checkpoint names: the detections come back bit for bit
    other, _ = _detector("tiny", seed=23)
    assert not torch.equal(other.forward(x[:3])[0], plain[0])
    assert weights.load_pointpillars(other, weights.pointpillars_state(m)) == []
    other.to(DEV)
    again = other.forward(x[:3])
    assert torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1])


def _logical(m):
    return neck_checks.logical(m, DEV)


def _neck_and_head_reference(m, x):
    """The RPN of pointpillars.py:367-621 (tests/neck_checks.py: every launch held to conv_contract.conv_stage on the device's own input,
    and the float64 chain with its accumulated bound.  Through sixteen randomly initialised layers that worst-case bound grows by the
    layers' sum |w| each time and ends far above the values; it is asserted because it is the bound that holds, and printed) and
    the three 1x1 heads restated the same way.
    -> (device neck output rebuilt from the single launches, (chain value, chain bound) of the neck, of the head, worst single-layer
    err / bound)"""
    stage = neck_checks.Stages()
    feat_d, (feat, fe) = neck_checks.neck_reference(m.neck, x, stage)
    heads = []
    for cm in m.bbox_head.children():
        wl, b = _logical(cm)
        n, h, w, c = feat.shape
        heads.append(stage(feat, fe, feat_d, wl, b, cc._plain(n, h, w, c, 1, 1, 0, cm.cout), 0, cm(feat_d)[..., :cm.cout]))
    return feat_d, (feat, fe), (torch.cat([v for v, _ in heads], 3), torch.cat([b for _, b in heads], 3)), stage.worst


def _check_net(tag, m, x, aux):
    feat_d, (feat, fe), (head, he), worst = _neck_and_head_reference(m, x)
    assert torch.equal(feat_d.view(torch.int16), aux["neck"].view(torch.int16))          # the single launches ARE the forward's
    print(f"{tag}: worst single-layer err / bound {worst:.3f}")
    for name, got, want, bound in (("neck", aux["neck"], feat, fe), ("head", aux["head"][..., :head.shape[3]], head, he)):
        err = (got.double() - want).abs()
        print(f"{tag} {name}: chain err {float(err.max()):.3g} on values up to {float(want.abs().max()):.3g}, accumulated bound up to "
              f"{float(bound.max()):.3g}, worst err / bound {float((err / bound).max()):.3g}")
        assert bool((err <= bound).all()), name


def test_tiny_neck_and_head_against_float64():
    m, _ = _detector("tiny")
    x, _ = _pseudo(3, m.grid_hw, 12)
    _, aux = m.forward(x, return_aux=True)
    _check_net("tiny", m, x, aux)


def test_car_config_runs_once_at_batch_2():
    m, cfg = _detector("car_xyres16")
    assert tuple(m.anchors.shape) == (107136, 7)
    x, _ = _pseudo(2, m.grid_hw, 13, fill=0.03)
    (dets, count), aux = m.forward(x, return_aux=True)
    torch.cuda.synchronize()
    assert aux["neck"].shape == (2, 248, 216, 384) and aux["head"].shape == (2, 248, 216, 24) and aux["scores"].shape == (2, 107136)
    _structure(dets, count, 300, 0.09, 1)
    _check_net("car", m, x, aux)
