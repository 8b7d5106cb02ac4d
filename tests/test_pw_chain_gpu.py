"""-m gpu: md_pw_chain (conv3 + residual + ReLU of one ResNet stage-2 bottleneck block and conv1 + ReLU of the next in one launch) against
the two md_conv2d launches it replaces on default dispatch -- bit for bit -- and y against the float64 contract of tests/conv_contract.py
within that contract's own bound.  Shapes: fewer tiles than the look-ahead (one ragged 32-pixel tile), two ragged tiles, image boundaries
inside tiles with one tile per workgroup, and 1050 tiles over 256 workgroups (unequal tile counts, a steady-state loop and a drain)."""
import functools

import pytest
import torch

from tests import conv_contract as cc
from tests.abi_cases_chain import CASES
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
SHAPES = [(1, 1, 31), (1, 5, 7), (3, 13, 21), (2, 100, 168)]


@functools.lru_cache(maxsize=None)
def _packs():
    from minddet_amd import nn_ops

    g = torch.Generator().manual_seed(1234)
    bn = lambda c: (torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1, torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5, 1e-5)
    w3 = torch.randn((512, 128, 1, 1), generator=g) * (2.0 / 128) ** 0.5
    w1 = torch.randn((128, 512, 1, 1), generator=g) * (2.0 / 512) ** 0.5
    pc3 = nn_ops.pack_conv(w3, bn=bn(512), relu=True).to(DEV)
    pc1 = nn_ops.pack_conv(w1, bn=bn(128), relu=True).to(DEV)
    pk = nn_ops.pack_pw_chain(pc3, pc1)
    assert pk is not None
    return pc3, pc1, pk


@functools.lru_cache(maxsize=None)
def _case(shape):
    """inputs and the two-launch reference of one shape, computed once and never written again"""
    from minddet_amd import nn_ops

    pc3, pc1, _ = _packs()
    n, h, w = shape
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + w)
    t2 = torch.randn((n, h, w, 128), generator=g).to(torch.bfloat16).to(DEV)
    res = torch.randn((n, h, w, 512), generator=g).to(torch.bfloat16).to(DEV)     # both signs: both ReLU outcomes occur
    y_ref = nn_ops.conv2d(t2, pc3, residual=res)
    t1_ref = nn_ops.conv2d(y_ref, pc1)
    torch.cuda.synchronize()
    return t2, res, y_ref, t1_ref


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_chain_equals_the_two_launches_bit_for_bit(shape):
    from minddet_amd import nn_ops

    t2, res, y_ref, t1_ref = _case(shape)
    y, t1 = nn_ops.pw_chain(t2, res, _packs()[2])
    torch.cuda.synchronize()
    frac_zero = (y_ref == 0).float().mean().item()
    assert 0.2 < frac_zero < 0.8, frac_zero                      # both ReLU outcomes
    ny, nt = int((y != y_ref).sum()), int((t1 != t1_ref).sum())
    print(f"{shape}: y mismatches {ny} / {y.numel()}, t1 mismatches {nt} / {t1.numel()}")
    assert torch.equal(y, y_ref), ny
    assert torch.equal(t1, t1_ref), nt


def test_three_repeated_calls_are_bit_equal():
    from minddet_amd import nn_ops

    t2, res, y_ref, t1_ref = _case(SHAPES[3])
    for _ in range(3):
        y, t1 = nn_ops.pw_chain(t2, res, _packs()[2])
        assert torch.equal(y, y_ref) and torch.equal(t1, t1_ref)


@pytest.mark.parametrize("shape", SHAPES[:3], ids=["x".join(map(str, s)) for s in SHAPES[:3]])
def test_y_is_within_the_float64_contract(shape):
    from minddet_amd import nn_ops

    pc3, _, pk = _packs()
    t2, res, _, _ = _case(shape)
    y, _ = nn_ops.pw_chain(t2, res, pk)
    n, h, w = shape
    geo = cc._plain(n, h, w, 128, 1, 1, 0, 512)
    wl = pc3.w[:512, :128].view(512, 1, 1, 128)
    want, bound = cc.conv_stage(t2, 0.0, wl, pc3.bias, geo, 1, res=res.double())
    err = (y.double() - want).abs()
    print(f"{shape}: worst err / bound {(err / bound).max().item():.4f}")
    assert bool((err <= bound).all())


def test_refusals_and_the_valid_row_on_the_device():
    from minddet_amd import _lib, nn_ops

    ops = CASES[0].operands
    dt = {"bfloat16": torch.bfloat16, "float32": torch.float32}
    ten = [torch.zeros(t.shape, dtype=dt[t.dtype], device=DEV) for t in ops]
    assert _lib.call("md_pw_chain", ten) == 0
    t2, res, _, _ = _case(SHAPES[1])
    pk = _packs()[2]

    def refused(tensors):
        with pytest.raises(_lib.MindDetHipError, match="rc=2"):
            _lib.call("md_pw_chain", tensors)

    y, t1 = torch.empty_like(res), torch.empty_like(t2)
    w = [pk.w3, pk.b3, pk.w1, pk.b1]
    refused([t2, res] + w + [res, t1])                          # y in place on the residual
    refused([t2, res] + w + [y, t2])                            # t1 in place on t2
    refused([t2[..., :64].contiguous(), res] + w + [y, t1])     # other channel counts
    wide = torch.zeros((1, 5, 7, 1024), dtype=torch.bfloat16, device=DEV)
    refused([t2, wide] + w + [y, t1])                           # a residual that is a channel slice of a wider tensor
    refused([t2, res] + w + [wide, t1])
    flat = torch.zeros(2 * res.numel(), dtype=torch.bfloat16, device=DEV)
    y_a, t1_a = flat[:res.numel()].view(res.shape), flat[512:512 + t2.numel()].view(t2.shape)
    refused([t2, res] + w + [y_a, t1_a])                        # the outputs overlap each other
    with pytest.raises(_lib.MindDetHipError):
        nn_ops.pw_chain(t2, res[..., :256].contiguous(), pk)


def test_backbone_features_with_the_chain_on_and_off_are_bit_identical(monkeypatch):
    from minddet_amd import _lib, graphs

    bb = graphs.ResNet(depth=50).to(DEV)
    x = torch.zeros((1, 96, 128, 8), dtype=torch.bfloat16, device=DEV)
    x[..., :3] = torch.randn((1, 96, 128, 3), generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).to(DEV)
    names, orig = [], _lib.call

    def record(name, tensors, extra=None, stream=None):
        names.append(name)
        return orig(name, tensors, extra=extra, stream=stream)

    monkeypatch.setattr(_lib, "call", record)
    monkeypatch.setattr(graphs, "PW_CHAIN", False)
    off = bb(x)
    n_off = (names.count("md_pw_chain"), names.count("md_conv2d"))
    del names[:]
    monkeypatch.setattr(graphs, "PW_CHAIN", True)
    on = bb(x)
    n_on = (names.count("md_pw_chain"), names.count("md_conv2d"))
    torch.cuda.synchronize()
    assert n_off[0] == 0 and n_on == (2, n_off[1] - 4), (n_off, n_on)      # two boundaries, each instead of two md_conv2d launches
    assert len(on) == len(off) == 4 and all(torch.equal(a, b) for a, b in zip(on, off))
