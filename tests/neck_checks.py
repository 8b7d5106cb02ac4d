"""Shared by test_pointpillars_gpu.py (KITTI) and test_centerpoint_conv_gpu.py (nuScenes): a graphs.RPN neck restated layer by layer in
float64 on the folded bf16 weights, every launch held to tests/conv_contract.py on the DEVICE's own input of that launch."""
import torch

from tests import conv_contract as cc
from tests.conv_checks import SENTINEL, check_guards, sentinel_out


def logical(m, device):
    """(folded weights as the kernel holds them: bf16 values, [cout, kh, kw, cin] float64; fp32 bias) of a ConvModule"""
    from minddet_amd import nn_ops

    w, b = nn_ops._fold_bn(m.weight, m.bias, m.bn)
    return w.to(torch.bfloat16).double().permute(0, 2, 3, 1).to(device), b.to(device)


class Stages:
    """stage(): one launch against conv_stage on the device's input (asserted, the worst err / bound kept per kind of launch), and
    the same conv appended to the float64 chain"""

    def __init__(self):
        self.worst, self.by_kind = 0.0, {}

    def __call__(self, t, e, td, wl, b, geo, relu, yd, kind="conv"):
        want, bound = cc.conv_stage(td.double(), 0.0, wl, b, geo, relu)             # this launch alone, on the device's input
        r = float(((yd.double() - want).abs() / bound).max())
        self.worst = max(self.worst, r)
        self.by_kind[kind] = max(self.by_kind.get(kind, 0.0), r)
        assert r <= 1.0, (geo, r)
        return cc.conv_stage(t, e, wl, b, geo, relu)


def _alone_in_concat(d, td, ud, c_off, channels):
    """the deblock's launches once more, into its channel slice of a sentinel-filled concat output: the slice is what the deblock gives
    alone, bit for bit; every other channel and the guard zones keep the sentinel"""
    n, h, w, _ = ud.shape
    out, flat = sentinel_out((n, h, w, channels), td.device)
    d(td, out=out, c_off=c_off)
    torch.cuda.synchronize()
    check_guards(flat)
    oi = out.view(torch.int16)
    assert torch.equal(oi[..., c_off:c_off + d.cout], ud.view(torch.int16)), c_off
    assert bool((oi[..., :c_off] == SENTINEL).all()) and bool((oi[..., c_off + d.cout:] == SENTINEL).all()), c_off


def neck_reference(neck, x, stage):
    """The RPN of pointpillars.py:367-621 / det3d's rpn.py:9-154 layer by layer through conv_contract.conv_stage, in two ways at once:
    * the chain: the exact value of the whole net and conv_contract's accumulated bound (fp32 accumulation, one bf16 rounding per
      layer, carried through the following layers' |w|);
    * layer by layer from the DEVICE's own input of each layer (the module run alone: the launch the neck makes): the bound of one
      conv on exact inputs, which is what pins each kernel launch (asserted in `stage`).
    A deblock is a k = stride conv (k = 1: pointwise; k > 1: the strided downsampling conv of a deblock stride below 1) or a
    k = stride Conv2dTranspose, whose s x s sub-pixel launches are 1x1 convs into the output pixels of one parity.
    -> (device neck output rebuilt from the single launches, (chain value, chain bound))"""
    from minddet_amd import graphs, nn_ops

    dev = x.device
    ups, ups_d = [], []
    t, e, td = x.double(), 0.0, x
    for i, blk in enumerate(neck.blocks):
        for cm in blk:
            wl, b = logical(cm, dev)
            n, h, w, _ = t.shape
            yd = cm(td)
            t, e = stage(t, e, td, wl, b, cc._plain(n, h, w, cm.cin, 3, cm.stride, 1, cm.cout), 1, yd)
            td = yd
        if i < neck.up_start:
            continue
        d = neck.deblocks[i - neck.up_start]
        n, h, w, _ = t.shape
        ud = d(td)
        if isinstance(d, graphs.DeconvModule):
            s = d.stride
            assert d.k == s and d.pad == 0
            wf, b = nn_ops._fold_bn(d.weight_t.permute(1, 0, 2, 3), None, d.bn)                     # [cout, cin, k, k]
            wf = wf.to(torch.bfloat16).double().to(dev)
            u = torch.zeros((n, h * s, w * s, d.cout), dtype=torch.float64, device=dev)
            ue = torch.zeros_like(u)
            for py in range(s):
                for px in range(s):
                    u[:, py::s, px::s], ue[:, py::s, px::s] = stage(t, e, td, wf[:, :, py, px][:, None, None, :], b.to(dev),
                                                                    cc._plain(n, h, w, d.cin, 1, 1, 0, d.cout), 1, ud[:, py::s, px::s],
                                                                    kind=f"deconv k{s} s{s}")
        else:
            assert d.k == d.stride and d.pad == 0
            wl, b = logical(d, dev)
            u, ue = stage(t, e, td, wl, b, cc._plain(n, h, w, d.cin, d.k, d.stride, 0, d.cout), 1, ud, kind=f"deblock conv k{d.k} s{d.stride}")
        _alone_in_concat(d, td, ud, sum(v.shape[3] for v in ups_d), neck.out_channels)
        ups.append((u, ue))
        ups_d.append(ud)
    feat, fe = torch.cat([u for u, _ in ups], 3), torch.cat([ue for _, ue in ups], 3)
    return torch.cat(ups_d, 3), (feat, fe)
