"""-m gpu: the reference-present graphs -- CenterNet-R18 (neck with Conv2dTranspose 4x4 s2 p1, fused heads,
sigmoid+clip, max-pool NMS, two-stage top-k, gather decode) and the CenterPoint RPN neck (strided conv /
Conv2dTranspose k=s deblocks writing a channel-concatenated output) -- against the torch/numpy oracle.
CenterNet's feature path and Conv2dTranspose are held to the float64 judge of tests/centernet_checks.py; decode indices: bit-exact from the
device head tensors.  CenterPoint's neck is held launch by launch to the float64 conv contract in tests/test_centerpoint_conv_gpu.py."""
import numpy as np
import pytest
import torch

from oracle import nets, np_ops
from tests import centernet_checks
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"


@pytest.mark.parametrize("k,s,p,cin,cout", [(4, 2, 1, 64, 64), (2, 2, 0, 128, 128), (4, 4, 0, 256, 128), (4, 2, 1, 16, 24)])
def test_conv_transpose_vs_torch(k, s, p, cin, cout):
    """the pack against the float64 fold and the launches against the scatter definition within conv_contract's bound, into a fresh output
    and into a channel slice of a sentinel buffer (tests/centernet_checks.py; more shapes in tests/test_centernet_chain_gpu.py)"""
    from minddet_amd import nn_ops

    g = torch.Generator().manual_seed(k * 10 + s)
    wt = torch.randn((cin, cout, k, k), generator=g) * (2.0 / (k * k * cin)) ** 0.5
    bn = (torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1, torch.randn(cout, generator=g) * 0.1,
          torch.rand(cout, generator=g) + 0.5, 1e-3)
    pct = nn_ops.pack_conv_transpose(wt, bn=bn, stride=s, pad=p, relu=True).to(DEV)
    x = torch.randn((2, 13, 17, cin), generator=g).to(torch.bfloat16)
    worst = centernet_checks.check_conv_transpose(pct, wt, bn, p, x.to(DEV), exact=False)
    print(f"conv_transpose2d k{k} s{s} p{p} {cin}->{cout} 2x13x17: worst err/bound {worst:.3f}")


def test_centerpoint_rpn_neck_shape_and_values():
    from minddet_amd import graphs

    # known answer from the reference's own smoke test (rpn.py:157-164): [4,64,512,512] -> [4,384,128,128];
    # run here at 1/4 size so that the fp32 oracle finishes in seconds: [1,64,128,128] -> [1,384,32,32]
    neck = graphs.RPN(num_input_features=64).to(DEV)
    assert neck.out_channels == 384
    g = torch.Generator().manual_seed(0)
    x = torch.randn((1, 128, 128, 64), generator=g).to(torch.bfloat16)
    y = neck(x.to(DEV)).float().cpu()
    assert y.shape == (1, 32, 32, 384)
    ref = nets.rpn_neck_forward(neck, x.float().permute(0, 3, 1, 2), quant=True).permute(0, 2, 3, 1)
    rms = ref.pow(2).mean().sqrt().item()
    err = (y - ref).abs().max().item()
    assert err <= 5e-2 * (rms + ref.abs().max().item() * 0.1), (err, rms)
    # full reference size: shape only
    y4 = neck(torch.zeros((4, 512, 512, 64), dtype=torch.bfloat16, device=DEV))
    assert y4.shape == (4, 128, 128, 384)


def test_centernet_end_to_end():
    from minddet_amd import graphs

    m = graphs.CenterNet(depth=18, num_classes=80).to(DEV)
    g = torch.Generator().manual_seed(1)
    x = torch.zeros((1, 256, 320, 8))
    x[..., :3] = torch.randn((1, 256, 320, 3), generator=g)
    xb = x.to(torch.bfloat16)
    det, aux = m.forward(xb.to(DEV), return_aux=True)
    torch.cuda.synchronize()
    assert det.shape == (1, 100, 6) and aux["hm"].shape == (1, 80, 64, 80)
    # the head tensor: the whole feature path against the float64 judge (tests/centernet_checks.py: the fold, every launch on the device's own
    # input, the fused heads against the unfused ones bit for bit, the chain's accumulated bound)
    out = centernet_checks.check_all(m, xb.to(DEV))
    centernet_checks.report("CenterNet-R18 1x256x320", out)
    assert torch.equal(aux["head"].view(torch.int16), out["head"].view(torch.int16))
    # decode from the DEVICE head tensors: indices / classes bit-exact, boxes to fp tolerance
    hm, wh, reg = aux["hm"].cpu().numpy(), aux["wh"].cpu().numpy(), aux["reg"].cpu().numpy()
    d_o, i_o, c_o = np_ops.centernet_decode(hm, wh, reg, 100)
    np.testing.assert_array_equal(aux["inds"].cpu().numpy(), i_o)
    np.testing.assert_array_equal(aux["cls"].cpu().numpy(), c_o)
    np.testing.assert_allclose(det.cpu().numpy(), d_o, rtol=1e-6, atol=1e-5)
    # sigmoid+clip bounds (utils.py:132-157)
    assert hm.min() >= 1e-4 - 1e-9 and hm.max() <= 1 - 1e-4 + 1e-7
