"""-m gpu: CenterPoint's conv path held to the float64 conv contract of tests/conv_contract.py, launch by launch.

1. md_conv2d_grouped (csrc/grouped.hip) through the C ABI on the cases of conv_checks.GROUPED_CASES -- the smallest shapes that reach each
   edge of the kernel's 8 x 32 pixel tile (one exact tile, one pixel over, smaller than a tile, ragged), every cout 1 .. 16, the header's
   64 groups, fewer work items than the eight workgroups of one launch round and a count that is no multiple of eight, the real head's
   36 groups -- in the contract's two data regimes (test_conv_production_gpu.py describes them): exact-integer data, bit for bit (here
   K <= 576 and |sum| < 2^11: fp32 is exact in any order, and ReLU or the identity leaves one bf16 rounding), and Gaussian data within
   conv_contract.gaussian_bound on every element.  The operands are packed from the header's text (conv_contract.pack_grouped), in
   one case with the groups' rows out of order between rows of NaN.  y starts as the bf16-NaN sentinel inside a sentinel buffer with
   guard zones: what the call must not write keeps the sentinel bit for bit, and no written element does.
2. CenterHead built from the nuScenes config, every launch alone on its DEVICE input against conv_stage on the folded bf16 weights: the
   shared conv, the merged 64 -> 2304 first conv, the grouped last conv (into a sentinel-filled head tensor: the channels past
   head_channels stay unwritten, every branch sits at task_offsets()), and the 36 per-branch md_conv2d launches of grouped=False.
3. CenterPoint's RPN neck (us_layer_strides 0.5, 1, 2) layer by layer through tests/neck_checks.py: 16 block convs, the k2 s2 strided
   conv deblock at c_off 0, the 1x1 deblock at c_off 128, the four sub-pixel launches of the k = s = 2 deconv at c_off 256; each
   deblock alone into a sentinel-filled 384-channel output; the neck's output equal to the single launches bit for bit.  The strided
   k2 s2 conv with c_off and the k = s deconv also in the exact regime.

The worst err / bound of each case is printed (`pytest -s`); where K is small the half-ulp term dominates the bound and is attained at
a bf16 tie, so ratios close to 1 are expected there."""
import os

import pytest
import torch

from tests import conv_contract as cc
from tests import neck_checks
from tests.conftest import has_gpu
from tests.conv_checks import GROUPED_CASES, REAL_COUTS, SENTINEL, Data, check, check_guards, grouped_operands, sentinel_out

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc.py")
MD_CONV_KERNEL_GROUPED = 10


def _detector(seed=7):
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(CFG)
    return build_detector(dict(cfg.model, seed=seed), cfg.train_cfg, cfg.test_cfg)


def _held(y, flat, ref, exact):
    """a sentinel-born output against a reference that is NaN where the call writes nothing -> worst err / bound (0: exact regime)"""
    check_guards(flat)
    want = ref if exact else ref[0]
    written = ~want.isnan()
    yi = y.view(torch.int16)
    assert bool((yi[~written] == SENTINEL).all()), "write outside the call's output region"
    assert not bool((yi[written] == SENTINEL).any()), "output element left unwritten"
    return check(y[written], want[written] if exact else (want[written], ref[1][written]), exact)


# ---------------------------------------------------------------------------------------------------------- 1. md_conv2d_grouped
@pytest.mark.parametrize("name", list(GROUPED_CASES))
def test_grouped_conv(name):
    from minddet_amd import _lib, nn_ops

    if name == "real_head":       # the cout table and the channel layout are CenterHead's own
        h = _detector().bbox_head
        assert [c2.cout for _, _, _, c2 in h.branches()] == REAL_COUTS and (h.head_channels + 7) // 8 * 8 == GROUPED_CASES[name]["Cy"]
        assert [h.offsets[t][n] for t, n, _, _ in h.branches()] == cc.grouped_attrs(3, REAL_COUTS)["y_off"]
    worst = 0.0
    for exact in (True, False):
        x, wls, biases, a, y_shape = grouped_operands(name, exact, DEV)
        own_rows = a["w_row"] != cc.grouped_attrs(a["k"], a["cout"])["w_row"]
        w, bias, rows = cc.pack_grouped(wls, biases, a["w_row"], fill=float("nan") if own_rows else 0.0)
        assert rows == a["w_row"]
        at = nn_ops._GroupedAttrs(a["k"], a["relu"], a["groups"], a["cin_g"], a["x_c_off"], 0)
        for g in range(a["groups"]):
            at.cout[g], at.y_off[g], at.w_row[g] = a["cout"][g], a["y_off"][g], a["w_row"][g]
        y, flat = sentinel_out(y_shape, DEV)
        _lib.call("md_conv2d_grouped", [x, w, bias, y], extra=at)
        torch.cuda.synchronize()
        assert _lib.lib().md_conv2d_last_kernel() == MD_CONV_KERNEL_GROUPED
        worst = max(worst, _held(y, flat, cc.reference_grouped(x, wls, biases, a, y_shape, exact=exact), exact))
    print(f"worst gaussian err/bound grouped {name}: {worst:.4f}")


# ------------------------------------------------------------------------------------------------------- 2. CenterHead, per launch
def _branch_operands(h):
    """per branch, in branches() order: (c2's logical weight [cout, 3, 3, 64] float64 of bf16 values, its fp32 bias)"""
    return [neck_checks.logical(c2, DEV) for _, _, _, c2 in h.branches()]


def test_center_head_launch_by_launch():
    from minddet_amd import nn_ops

    h = _detector(3).bbox_head.to(DEV)
    br = h.branches()
    assert len(br) == 36 and h.head_channels == 70
    g = torch.Generator().manual_seed(21)
    x = (torch.randn((2, 19, 37, 384), generator=g) * 0.7).clamp(min=0).to(torch.bfloat16).to(DEV)      # post-ReLU features
    N, H, W, _ = x.shape
    stage = neck_checks.Stages()
    # the shared conv: 3x3, 384 -> 64, bias + BN + ReLU
    sh = h.shared_conv(x)
    wl, b = neck_checks.logical(h.shared_conv, DEV)
    stage(x.double(), 0.0, x, wl, b, cc._plain(N, H, W, 384, 3, 1, 1, 64), 1, sh, kind="shared 384->64")
    # the 36 first convs as one md_conv2d 64 -> 2304 (K = 576): branch i's channels at 64 i, each folded as its own ConvModule
    mid = nn_ops.conv2d(sh, h._first)
    assert mid.shape == (N, H, W, 64 * len(br))
    firsts = [neck_checks.logical(c1, DEV) for _, _, c1, _ in br]
    stage(sh.double(), 0.0, sh, torch.cat([w_ for w_, _ in firsts]), torch.cat([b_ for _, b_ in firsts]),
          cc._plain(N, H, W, 64, 3, 1, 1, 64 * len(br)), 1, mid, kind="merged 64->2304")
    # the grouped last conv into a sentinel-filled head tensor: every branch at task_offsets(), channels past head_channels unwritten
    seconds = _branch_operands(h)
    offs = h.task_offsets(grouped=True)
    a = cc.grouped_attrs(3, [c2.cout for _, _, _, c2 in br], y_offs=[offs[t][n] for t, n, _, _ in br])
    cy = (h.head_channels + 7) // 8 * 8
    head, flat = sentinel_out((N, H, W, cy), DEV)
    nn_ops.conv2d_grouped(mid, h._second, head)
    torch.cuda.synchronize()
    ref = cc.reference_grouped(mid, [w_ for w_, _ in seconds], [b_ for _, b_ in seconds], a, head.shape, exact=False)
    assert bool(ref[0][..., h.head_channels:].isnan().all()) and not bool(ref[0][..., :h.head_channels].isnan().any())
    r_grouped = _held(head, flat, ref, False)
    # the per-branch form: branch i's md_conv2d alone reads slice 64 i and writes the 8-channel slot 8 i (channels past cout: zero rows)
    offs8 = h.task_offsets(grouped=False)
    assert [offs8[t][n] for t, n, _, _ in br] == [8 * i for i in range(len(br))]
    head8 = torch.empty((N, H, W, 8 * len(br)), dtype=torch.bfloat16, device=DEV)
    r_branch = 0.0
    for i, ((_, _, _, c2), (wl, b)) in enumerate(zip(br, seconds)):
        out, flat8 = sentinel_out(head8.shape, DEV)
        nn_ops.conv2d(mid, c2.packed, out=out, c_off=8 * i, x_c_off=64 * i)
        torch.cuda.synchronize()
        wl8, b8 = torch.zeros((8, 3, 3, 64), dtype=torch.float64, device=DEV), torch.zeros((8,), dtype=torch.float32, device=DEV)
        wl8[:c2.cout], b8[:c2.cout] = wl, b
        geo = cc.Geometry(3, 3, 1, 1, 1, H, W, 1, 0, 0, 8 * i, 8, 64 * i, 64, tuple(head8.shape))
        v, e = cc.conv_stage(mid.double(), 0.0, wl8, b8, geo, 0)
        want, bound = torch.full(head8.shape, float("nan"), dtype=torch.float64, device=DEV), torch.full(head8.shape, float("nan"), dtype=torch.float64, device=DEV)
        cc.out_view(want, geo)[...], cc.out_view(bound, geo)[...] = v, e
        r_branch = max(r_branch, _held(out, flat8, (want, bound), False))
        head8[..., 8 * i:8 * i + 8] = out[..., 8 * i:8 * i + 8]
    # the head's own passes are these launches
    for grouped, want in ((True, head[..., :h.head_channels]), (False, head8)):
        got, got_sh = h(x, grouped=grouped)
        assert torch.equal(got_sh.view(torch.int16), sh.view(torch.int16))
        assert torch.equal(got[..., :want.shape[3]].contiguous().view(torch.int16), want.contiguous().view(torch.int16)), grouped
    print("worst err/bound CenterHead: " + ", ".join(f"{k} {v:.4f}" for k, v in stage.by_kind.items()) +
          f", grouped last conv {r_grouped:.4f}, per-branch last convs {r_branch:.4f}")


# ---------------------------------------------------------------------------------------------------------- 3. the neck, per launch
def test_centerpoint_neck_launch_by_launch():
    neck = _detector(5).neck.to(DEV)
    assert [type(d).__name__ for d in neck.deblocks] == ["ConvModule", "ConvModule", "DeconvModule"]
    assert [(d.k, d.stride, d.cout) for d in neck.deblocks] == [(2, 2, 128), (1, 1, 128), (2, 2, 128)] and neck.up_start == 0
    g = torch.Generator().manual_seed(22)
    x = torch.rand((1, 104, 72, 64), generator=g) * 1.5
    x = (x * (torch.rand((1, 104, 72, 1), generator=g) < 0.3)).to(torch.bfloat16).to(DEV)              # a sparse pseudo-image
    stage = neck_checks.Stages()
    feat_d, (feat, fe) = neck_checks.neck_reference(neck, x, stage)
    assert sum(len(b) for b in neck.blocks) == 16 and set(stage.by_kind) == {"conv", "deblock conv k2 s2", "deblock conv k1 s1", "deconv k2 s2"}
    y = neck(x)
    torch.cuda.synchronize()
    assert y.shape == (1, 26, 18, 384) and torch.equal(y.view(torch.int16), feat_d.view(torch.int16))   # the single launches ARE the neck's
    err = (y.double() - feat).abs()
    assert bool((err <= fe).all())                                                                         # the chain's accumulated bound
    print("worst err/bound CenterPoint neck: " + ", ".join(f"{k} {v:.4f}" for k, v in stage.by_kind.items()) +
          f"; chain err {float(err.max()):.3g} on values up to {float(feat.abs().max()):.3g}, accumulated bound up to {float(fe.max()):.3g}")


@pytest.mark.parametrize("c_off", [0, 128])
def test_strided_k2s2_conv_with_c_off_exact(c_off):
    """the first deblock's form: a k = 2, stride 2, pad 0 conv 64 -> 128 into channels [c_off, c_off + 128) of a 384-channel output;
    13 x 17 -> 6 x 8: the last input row and column are not read"""
    from minddet_amd import nn_ops

    d = Data(True, 4100 + c_off, DEV)
    x = d.act((2, 13, 17, 64))
    wl, b = d.weight((128, 2, 2, 64), 256), d.bias(128, 128)
    for relu in (False, True):
        pc = nn_ops.pack_conv(wl.float().permute(0, 3, 1, 2).cpu(), bias=b.cpu(), stride=2, pad=0, relu=relu).to(DEV)
        y, flat = sentinel_out((2, 6, 8, 384), DEV)
        nn_ops.conv2d(x, pc, out=y, c_off=c_off)
        torch.cuda.synchronize()
        geo = cc.Geometry(2, 2, 2, 0, 0, 6, 8, 1, 0, 0, c_off, 128, 0, 64, (2, 6, 8, 384))
        want = torch.full(y.shape, float("nan"), dtype=torch.float64, device=DEV)
        cc.out_view(want, geo)[...] = cc.conv_stage(x, None, wl, b, geo, int(relu))[0]
        _held(y, flat, want, True)


def test_k_equals_s_deconv_with_c_off_exact():
    """the last deblock's form: Conv2dTranspose k = s = 2, 64 -> 128, as four sub-pixel launches into channels [256, 384) of a
    384-channel output: output pixel (2 i + py, 2 j + px) = bf16(relu(b + sum_ci x[i, j, ci] wt[ci, :, py, px]))"""
    from minddet_amd import nn_ops

    d = Data(True, 4200, DEV)
    x = d.act((2, 13, 17, 64))
    wt = d.weight((64, 128, 2, 2), 64)                                   # Conv2dTranspose layout [cin, cout, k, k]
    b = d.bias(128, 128)
    pct = nn_ops.pack_conv_transpose(wt.float().cpu(), bias=b.cpu(), stride=2, pad=0, relu=True).to(DEV)
    y, flat = sentinel_out((2, 26, 34, 384), DEV)
    nn_ops.conv_transpose2d(x, pct, out=y, c_off=256)
    torch.cuda.synchronize()
    want = torch.full(y.shape, float("nan"), dtype=torch.float64, device=DEV)
    for py in range(2):
        for px in range(2):
            geo = cc.Geometry(1, 1, 1, 0, 0, 13, 17, 2, py, px, 256, 128, 0, 64, tuple(y.shape))
            cc.out_view(want, geo)[...] = cc.conv_stage(x, None, wt[:, :, py, px].t()[:, None, None, :], b, geo, 1)[0]
    assert not bool(want[..., 256:].isnan().any())
    _held(y, flat, want, True)
