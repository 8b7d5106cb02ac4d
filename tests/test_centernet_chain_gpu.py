"""-m gpu: graphs.CenterNet's feature path held to the float64 judge of tests/centernet_checks.py (which derives every bound and says which
condition pins what; tests/test_centernet_chain_cpu.py judges the judge): the fold of every conv against the float64 fold, the fused heads'
weights and outputs against the unfused ones, every launch alone on the device's own input, model.features against the single launches bit
for bit, and the float64 chain with conv_contract's accumulated bound, over the whole head tensor.

* configs/centernet/centernet_tiny_train.py at B = 2 (input 64 x 96, a 16 x 24 map), with dcn=True and with dcn=False;
* graphs.CenterNet(depth=18, num_classes=80) at 1 x 128 x 192 (the smallest input on which every stage keeps a map of at least 4 x 6 and the
  stem layout's H % 16, W % 64 rule holds), in the 8-channel layout and through nn_ops.to_stem_layout (md_stem_pool);
* the tiny model after three steps of head_trainer() on the fixed batch of tests/test_cn_head_train_gpu.py: features() of the trained shadow
  weights equals features() after to() (sync_modules -> fuse_heads -> repack) bit for bit, and the repacked model passes every check;
* nn_ops.conv_transpose2d on its own through the scatter definition: (k, s, p) in (4, 2, 1), (2, 2, 0), (4, 4, 0) x inputs 1x1, 1x7, 5x1, 5x7,
  13x17 (batch 2) x (cin, cout) in (16, 24), (64, 64), (256, 128), in conv_contract's exact regime (bit for bit) and the gaussian regime
  (cc.gaussian_bound), each into a fresh output and into channels [8, 8 + cout) of a NaN-sentinel [.., cout + 40] tensor with guard zones.

Each case prints its worst err / bound per kind of launch and the worst chain ratio (`pytest -s`).  Measured on an MI355X
(worst err / bound per kind of launch):
    case                         chain    7x7   3x3s2  3x3s1  3x3+res  1x1ds  dcn-off  cols   dcn-GEMM  deconv  head3x3  head1x1  head1  head2
    tiny 2x64x96 dcn=True        1.6e-36  0.968 0.900  0.906  0.972    0.995  0.909    1.000  0.844     0.986   0.945    0.996    0.945  0.990
    tiny 2x64x96 dcn=False       3.0e-34  0.968 0.900  0.906  0.972    0.995  -        -      -         0.971   0.939    0.993    0.939  0.983
    r18 nc80 1x128x192 c8        1.2e-36  0.966 0.921  0.929  0.962    0.995  0.864    1.000  0.857     0.982   0.954    0.998    0.954  0.993
    r18 nc80 1x128x192 stem      1.3e-36  0.984 0.921  0.929  0.962    0.995  0.864    1.000  0.857     0.982   0.954    0.998    0.954  0.993
    tiny after three head steps  4.0e-33  0.965 0.920  0.928  0.974    0.995  -        -      -         0.976   0.981    0.996    0.981  0.992
(7x7 of the stem row: md_stem_pool.  The max pool, the DCN module against its three launches, fused == unfused, the pad channels and
features == launches hold bit for bit everywhere, so the K order of the fused 3x3 does not change the accumulation: no one-ulp allowance is
used.  A launch ratio near 1 is an output next to a bf16 tie, where half an ulp is the whole bound; `cols` is sc.check's figure for
md_deform_cols.  The chain bound is conv_contract's worst case through some twenty layers and ends 33 to 36 orders above the error: it
holds, and pins nothing; the launch conditions on the heads do -- see tests/centernet_checks.py.)
conv_transpose2d alone, exact regime bit for bit in all 45 cases; worst gaussian err / bound per (k, s, p) x (16->24, 64->64, 256->128):
    (4, 2, 1): 0.995 0.974 0.835    (2, 2, 0): 0.999 0.994 0.968    (4, 4, 0): 0.999 0.996 0.971
The whole file runs in about 7 s, no test above 2 s."""
import os

import pytest
import torch

from tests import centernet_checks as cn
from tests.conftest import has_gpu
from tests.conv_checks import Data

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny(dcn):
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centernet", "centernet_tiny_train.py"))
    return build_detector(dict(cfg.model, dcn=dcn), cfg.train_cfg, cfg.test_cfg).to(DEV)


def images(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros((n, h, w, 8))
    x[..., :3] = torch.randn((n, h, w, 3), generator=g)
    return x.to(torch.bfloat16).to(DEV)


def _kinds(out, dcn, stem=False):
    want = {"conv 3x3 s1", "conv 3x3 s2", "conv 1x1 s2 downsample", "conv 3x3 s1 + residual", "deconv k4 s2 p1", "head 3x3", "head 1x1",
            "head1 (fused 3x3)", "head2 (fused 1x1)"}
    want |= {"md_stem_pool"} if stem else {"conv 7x7 s2", "maxpool 3x3 s2"}
    want |= {"dcn offset conv", "md_deform_cols", "dcn GEMM K=9C", "dcn module == its launches"} if dcn else set()
    assert set(out["launches"]) == want, set(out["launches"]) ^ want


@pytest.mark.parametrize("dcn", [True, False], ids=["dcn", "plain"])
def test_tiny_config(dcn):
    m = tiny(dcn)
    out = cn.check_all(m, images(2, 64, 96, 11))
    assert tuple(out["head"].shape) == (2, 16, 24, 16)
    _kinds(out, dcn)
    cn.report(f"tiny 2x64x96 dcn={dcn}", out)


@pytest.mark.parametrize("layout", ["c8", "stem"])
def test_r18_80_classes(layout):
    from minddet_amd import graphs, nn_ops

    m = graphs.CenterNet(depth=18, num_classes=80).to(DEV)
    x = images(1, 128, 192, 12)
    assert nn_ops.stem_layout_ok(128, 192)
    out = cn.check_all(m, nn_ops.to_stem_layout(x) if layout == "stem" else x)
    assert tuple(out["head"].shape) == (1, 32, 48, 88)
    _kinds(out, True, layout == "stem")
    cn.report(f"r18 nc80 1x128x192 {layout}", out)


def test_trained_head():
    from tests.test_cn_head_train_gpu import LR, batch, build

    net, _ = build()
    inp, ex = batch()
    before = net.features(inp).clone()
    tr = net.head_trainer()
    for _ in range(3):
        tr.train_step(inp, ex, lr=LR, beta1=0.9)
    trained = net.features(inp).clone()                       # head1 / head2 read the trainer's bf16 shadow of the masters
    assert not torch.equal(trained, before)
    net.to(DEV)                                               # sync_modules -> fuse_heads -> repack
    out = cn.check_all(net, inp)
    assert torch.equal(out["head"].view(torch.int16), trained.view(torch.int16)), "the repacked heads differ from the trained ones"
    cn.report("tiny 2x64x96 after three head steps", out)


@pytest.mark.parametrize("cin,cout", [(16, 24), (64, 64), (256, 128)])
@pytest.mark.parametrize("ksp", [(4, 2, 1), (2, 2, 0), (4, 4, 0)], ids=lambda v: "k%d_s%d_p%d" % v)
def test_conv_transpose_scatter(ksp, cin, cout):
    from minddet_amd import graphs, nn_ops

    k, s, p = ksp
    worst = 0.0
    for i, hw in enumerate(((1, 1), (1, 7), (5, 1), (5, 7), (13, 17))):
        for exact in (True, False):
            d = Data(exact, 7000 + 100 * k + 10 * i + cin + int(exact), DEV)
            x = d.act((2,) + hw + (cin,))
            if exact:                                         # weights in {-1, 0, 1}, no BatchNorm: every fp32 partial sum is exact
                wt, bn = d.weight((cin, cout, k, k), k).float().cpu(), None
            else:
                init = graphs.ParamInit(k * 10 + s + i)
                wt, bn = init.conv(cin, cout, k, (2.0 / (k * k * cin / (s * s))) ** 0.5), init.bn(cout, 1e-3)
            pct = nn_ops.pack_conv_transpose(wt, bn=bn, stride=s, pad=p, relu=True).to(DEV)
            worst = max(worst, cn.check_conv_transpose(pct, wt, bn, p, x, exact))
    print(f"conv_transpose2d k{k} s{s} p{p} {cin}->{cout}: worst err/bound (gaussian) {worst:.3f}")
