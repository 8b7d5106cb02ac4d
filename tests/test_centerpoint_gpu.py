"""-m gpu: the CenterPoint detector (graphs.PointPillars: RPN neck -> CenterHead -> CenterHeadPost per task -> task merge) and its new
kernel, md_conv2d_grouped (csrc/grouped.hip).
(a) the grouped op against fp32 F.conv2d(groups=G) on bf16-rounded operands, bound: one output rounding (half a bf16 ulp) + 1e-4;
(b) the grouped op against the per-head md_conv2d form: at most 1 bf16 ulp apart on every element;
(c) the CenterHead head tensor against the torch oracle (conv_module(quant=True) per branch);
(d) the known answer of center_head.py:490-491: [4,512,512,64] -> neck [4,128,128,384] -> shared [4,128,128,64];
(e) the detector end to end at B = 2: decode against np_ops.centerpoint_decode away from the score threshold, then TopK order, NMS keep
    lists, counts and the merged dets / labels / count bit-exact against the oracle and the merge rule of tools_ms/eval.py:84-111.
The grouped op and every CenterHead launch are held to the float64 conv contract in tests/test_centerpoint_conv_gpu.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from oracle import nets, np_ops
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc.py")
SENTINEL = -12352.0      # exactly representable in bf16 (0xC641)
# the 36 branches of the nuScenes model: per task reg 2, height 1, dim 3, rot 2, vel 2, hm 1 | 2
REAL_COUTS = [c for nc in (1, 2, 2, 1, 2, 2) for c in (2, 1, 3, 2, 2, nc)]


def _detector(seed=7):
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(CFG)
    return build_detector(dict(cfg.model, seed=seed), cfg.train_cfg, cfg.test_cfg), cfg


def _convs(couts, k, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for c in couts:
        w = torch.randn((c, 64, k, k), generator=g) * (1.0 / (8 * k))
        b = torch.randn((c,), generator=g) * 0.1
        bn = (torch.rand((c,), generator=g) + 0.5, torch.randn((c,), generator=g) * 0.1, torch.randn((c,), generator=g) * 0.1,
              torch.rand((c,), generator=g) + 0.5, 1e-5)
        out.append((w, b, bn))
    return out


def _grouped_ref(xb, pk, x_c_off, images):
    """fp32 F.conv2d(groups=G) on the bf16 operands (weights padded to 16 rows per group) -> per group [n, cout_g, H, W]"""
    G, k = pk.groups, pk.k
    wf = torch.zeros((G * 16, 64, k, k))
    bf = torch.zeros((G * 16,))
    w = pk.w.float().cpu().view(-1, k, k, 64).permute(0, 3, 1, 2)       # K order (tap, ci) -> [R, 64, k, k]
    for g in range(G):
        r, c = pk.w_rows[g], pk.couts[g]
        wf[16 * g:16 * g + c] = w[r:r + c]
        bf[16 * g:16 * g + c] = pk.bias.cpu()[r:r + c]
    x = xb[images, :, :, x_c_off:x_c_off + 64 * G].float().permute(0, 3, 1, 2)
    y = F.conv2d(x, wf, bf, padding=k // 2, groups=G)
    if pk.relu:
        y = torch.relu(y)
    return [y[:, 16 * g:16 * g + pk.couts[g]] for g in range(G)]


def _run_grouped_case(N, H, W, couts, k=3, x_c_off=0, extra_c=0, y_offs=None, Cy=None, relu=False, images=None, seed=0):
    from minddet_amd import _lib, nn_ops

    G = len(couts)
    pk = nn_ops.pack_conv2d_grouped(_convs(couts, k, seed), y_offs=y_offs, relu=relu).to(DEV)
    Cy = Cy if Cy is not None else (sum(couts) + 7) // 8 * 8
    C = x_c_off + 64 * G + extra_c
    g = torch.Generator().manual_seed(seed + 1)
    xb = torch.randn((N, H, W, C), generator=g).to(torch.bfloat16)
    y = torch.full((N, H, W, Cy), SENTINEL, dtype=torch.bfloat16, device=DEV)
    nn_ops.conv2d_grouped(xb.to(DEV), pk, y, x_c_off=x_c_off)
    torch.cuda.synchronize()
    assert _lib.lib().md_conv2d_last_kernel() == 10
    images = list(range(N)) if images is None else images
    yd = y.float().cpu()
    refs = _grouped_ref(xb, pk, x_c_off, images)
    covered = torch.zeros(Cy, dtype=torch.bool)
    for gi in range(G):
        o, c = pk.y_offs[gi], pk.couts[gi]
        covered[o:o + c] = True
        got = yd[images, :, :, o:o + c].permute(0, 3, 1, 2)
        ref = refs[gi]
        bound = ref.abs() * 2.0 ** -8 + 1e-4
        err = (got - ref).abs()
        assert (err <= bound).all(), (gi, float((err - bound).max()))
    # the contract for channels no group covers: left untouched
    assert (yd[..., ~covered] == SENTINEL).all()
    return pk, xb, y


def test_grouped_real_head_shape():
    # G = 36 at 4 x 128 x 128 with the real cout table and CenterHead's channel layout (reference on two of the four images)
    h = _detector()[0].bbox_head
    y_offs = [h.offsets[t][n] for t, n, _, _ in h.branches()]
    assert [c2.cout for _, _, _, c2 in h.branches()] == REAL_COUTS
    _run_grouped_case(4, 128, 128, REAL_COUTS, y_offs=y_offs, Cy=72, images=[0, 3])


def test_grouped_ragged_and_small_shapes():
    _run_grouped_case(2, 19, 37, [3, 1, 2, 16, 5])                          # ragged H / W (partial tiles in both directions)
    _run_grouped_case(1, 8, 32, [2, 1])                                     # N = 1, one exact tile
    _run_grouped_case(1, 5, 3, [4], relu=True)                              # smaller than a tile, ReLU
    _run_grouped_case(2, 24, 40, [2, 3, 1], x_c_off=128, extra_c=64)         # x_c_off != 0 on a wider tensor
    _run_grouped_case(1, 16, 48, [2, 3, 1, 2], y_offs=[21, 3, 40, 9], Cy=48)  # non-contiguous, out-of-order y_off, gaps (sentinel)
    _run_grouped_case(1, 12, 33, list(range(1, 17)))                        # cout_g 1 .. 16
    _run_grouped_case(2, 19, 37, [3, 1, 2, 16], k=1, y_offs=[0, 30, 8, 12], Cy=32)  # k = 1


def _ulp_dist(a, b):
    """distance in bf16 units in the last place between two bf16 tensors (ordered-integer view of the bit patterns)"""
    def ordered(t):
        i = t.view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -32768 - i, i)
    return (ordered(a) - ordered(b)).abs()


def test_grouped_against_per_head_md_conv2d():
    from minddet_amd import nn_ops

    couts = REAL_COUTS
    convs = _convs(couts, 3, 5)
    pk = nn_ops.pack_conv2d_grouped(convs, relu=False).to(DEV)
    g = torch.Generator().manual_seed(6)
    x = torch.randn((2, 128, 128, 64 * len(couts)), generator=g).to(torch.bfloat16).to(DEV)
    y = torch.empty((2, 128, 128, 72), dtype=torch.bfloat16, device=DEV)
    nn_ops.conv2d_grouped(x, pk, y)
    worst = 0
    for gi, (w, b, bn) in enumerate(convs):
        pc = nn_ops.pack_conv(w, bias=b, bn=bn, pad=1).to(DEV)
        yh = nn_ops.conv2d(x, pc, x_c_off=64 * gi)                          # slice input, 8-channel output
        o, c = pk.y_offs[gi], couts[gi]
        d = _ulp_dist(y[..., o:o + c], yh[..., :c])
        worst = max(worst, int(d.max()))
    assert worst <= 1, worst


def _pseudo_image(B, frac, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn((B, 512, 512, 64), generator=g))
    mask = torch.rand((B, 512, 512, 1), generator=g) < frac
    return (x * mask).to(torch.bfloat16)


def test_center_head_against_oracle():
    m, _ = _detector(3)
    h = m.bbox_head.to(DEV)
    g = torch.Generator().manual_seed(4)
    x = torch.randn((1, 24, 40, 384), generator=g).to(torch.bfloat16)
    for grouped in (True, False):
        head, shared = h(x.to(DEV), grouped=grouped)
        torch.cuda.synchronize()
        xs = nets.conv_module(h.shared_conv, x.float().permute(0, 3, 1, 2), quant=True)
        got_sh = shared.float().cpu().permute(0, 3, 1, 2)
        assert (got_sh - xs).abs().max().item() <= 2e-2 * (1 + xs.abs().max().item())
        hd = head.float().cpu().permute(0, 3, 1, 2)
        offs = h.task_offsets(grouped=grouped)
        for t, hn, c1, c2 in h.branches():
            ref = nets.conv_module(c2, nets.conv_module(c1, xs, quant=True), quant=True)
            o = offs[t][hn]
            got = hd[:, o:o + c2.cout]
            assert (got - ref).abs().max().item() <= 3e-2 * (1 + ref.abs().max().item()), (grouped, t, hn)
            assert (got - ref).abs().mean().item() <= 2e-3 * (1 + ref.abs().max().item()), (grouped, t, hn)


def test_known_answer_shapes():
    m, _ = _detector(5)
    m.to(DEV)
    x = torch.zeros((4, 512, 512, 64), dtype=torch.bfloat16, device=DEV)
    feat = m.neck(x)
    head, shared = m.bbox_head(feat)
    torch.cuda.synchronize()
    assert tuple(feat.shape) == (4, 128, 128, 384)
    assert tuple(shared.shape) == (4, 128, 128, 64)
    assert tuple(head.shape) == (4, 128, 128, 72)


def test_detector_end_to_end():
    from minddet_amd import det_ops

    m, cfg = _detector(9)
    m.to(DEV)
    tc = cfg.test_cfg
    B = 2
    x = _pseudo_image(B, 0.1, 11).to(DEV)
    (dets, count), aux = m.forward(x, return_aux=True)
    torch.cuda.synchronize()
    assert tuple(dets.shape) == (B, 6 * 83, 11) and dets.dtype == torch.float32 and count.dtype == torch.int32
    head = aux["head"]
    hf = head.float().cpu().numpy()
    h = m.bbox_head
    merged = [[] for _ in range(B)]
    flag = 0
    for t, (off, nc) in enumerate(zip(h.task_offsets(), h.num_classes)):
        (boxes, scores, labels, cnt), ax = det_ops.CenterHeadPost(off, nc, tc)(head, return_aux=True)
        # the detector's per-task outputs are these
        for a, b in zip(aux["tasks"][t], (boxes, scores, labels, cnt)):
            assert torch.equal(a, b)
        s_o, l_o, b_o, nb_o, mask_o = np_ops.centerpoint_decode(hf, off, nc, tc)
        s_d, l_d = ax["scores"].cpu().numpy(), ax["labels"].cpu().numpy()
        near = np.abs(np.where(mask_o, s_o, 1.0) - tc["score_threshold"]) < 1e-5
        assert ((s_d > -1) == mask_o)[~near].all()
        both = (s_d > -1) & mask_o
        np.testing.assert_allclose(s_d[both], s_o[both], rtol=2e-6, atol=1e-7)
        assert (l_d[both] == l_o[both]).mean() > 0.9999
        np.testing.assert_allclose(ax["boxes"].cpu().numpy()[both], b_o[both], rtol=3e-6, atol=2e-5)
        np.testing.assert_allclose(ax["nms_boxes"].cpu().numpy()[both], nb_o[both], rtol=3e-6, atol=2e-5)
        nbd, bxd = ax["nms_boxes"].cpu().numpy(), ax["boxes"].cpu().numpy()
        for b in range(B):
            v, order = np_ops.topk_desc_stable(s_d[b], tc["nms"]["nms_pre_max_size"])
            np.testing.assert_array_equal(ax["order"].cpu().numpy()[b], order)
            keep_o, num_o = oracle.nms_rot_aot(nbd[b][order], tc["nms"]["nms_iou_threshold"])
            np.testing.assert_array_equal(ax["keep"].cpu().numpy()[b], keep_o)
            assert int(ax["num_out"][b]) == num_o
            c = min(num_o, int((v > -1).sum()), tc["nms"]["nms_post_max_size"])
            assert int(cnt[b]) == c
            sc = v[keep_o[:c]]
            np.testing.assert_array_equal(scores.cpu().numpy()[b, :c], sc)
            size = int((sc > 0).sum())                                   # eval.py:84-111
            rows = np.zeros((size, 11), np.float32)
            rows[:, :9] = bxd[b][order][keep_o[:size]]
            rows[:, 9] = sc[:size]
            rows[:, 10] = l_d[b][order][keep_o[:size]] + flag
            merged[b].append(rows)
        flag += nc
    got, cnt_d = dets.cpu().numpy(), count.cpu().numpy()
    for b in range(B):
        ref = np.concatenate(merged[b], 0)
        assert int(cnt_d[b]) == len(ref)
        np.testing.assert_array_equal(got[b, :len(ref)], ref)
        assert (got[b, len(ref):] == 0).all()
    assert int(count.sum()) > 0
