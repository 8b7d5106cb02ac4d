"""-m gpu: md_pw_chain (conv3 + residual + ReLU of one ResNet stage-2 bottleneck block and conv1 + ReLU of the next in one launch) against
the two md_conv2d launches it replaces on default dispatch -- bit for bit -- and y against the float64 contract of tests/conv_contract.py
within that contract's own bound.  Shapes: fewer tiles than the look-ahead (one ragged 32-pixel tile), two ragged tiles, image boundaries
inside tiles with one tile per workgroup, and 1050 tiles over 256 workgroups (unequal tile counts, a steady-state loop and a drain).

Both outputs against conv_contract.reference_pw_chain, through the C ABI into NaN-sentinel outputs with guard zones (every element written,
nothing outside), on those shapes and two more that give a workgroup 1 or 2 and 3 or 4 tiles (the ring drains before it is full): an exact
regime on integer data, y and t1 bit for bit with no tolerance, and a Gaussian regime, y within conv3's bound and t1 within conv1's bound
on the device's own y."""
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
    # once more into sentinel-filled outputs: a call that wrote nothing cannot pass on what an earlier call left in a reused block
    pk = _packs()[2]
    y, t1 = _sentinel_call(t2, res, pk.w3, pk.b3, pk.w1, pk.b1)
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


# ---------------------------------------------------------------------------------------------------------------------------------
# both outputs against the float64 contract (conv_contract.reference_pw_chain), through the C ABI into sentinel outputs
# ---------------------------------------------------------------------------------------------------------------------------------
# + 304 tiles on 256 workgroups (1 or 2 tiles each) and 774 tiles (3 or 4 each: the look-ahead PC_D = 3 and the ring size), both with a
# ragged last tile
ALL_SHAPES = SHAPES + [(1, 97, 100), (1, 131, 189)]
_IDS = ["x".join(map(str, s)) for s in ALL_SHAPES]


def _sentinel_call(t2, res, w3, b3, w1, b1):
    """one md_pw_chain launch into NaN-sentinel outputs with guard zones: the guard zones stay intact and every element is written"""
    from minddet_amd import _lib
    from tests.conv_checks import SENTINEL, check_guards, sentinel_out

    y, fy = sentinel_out(tuple(res.shape), DEV)
    t1, ft = sentinel_out(tuple(t2.shape), DEV)
    _lib.call("md_pw_chain", [t2, res, w3, b3, w1, b1, y, t1])
    torch.cuda.synchronize()
    check_guards(fy)
    check_guards(ft)
    assert not bool((y.view(torch.int16) == SENTINEL).any()), "y element left unwritten"
    assert not bool((t1.view(torch.int16) == SENTINEL).any()), "t1 element left unwritten"
    return y, t1


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_IDS)
def test_exact_regime_both_outputs_bit_for_bit(shape):
    """Integer data, exact in fp32 in any summation order: y AND t1 equal the float64 result rounded where the header rounds, bit for
    bit -- the independent check of GEMM 2's 16x16x32 MFMA path (its B operand is the y tile in LDS).
    |t2| <= 2, |res| <= 8, weights {-1, 0, 1}, integer biases.  conv3's sum is an integer of standard deviation 13, which bf16 holds
    exactly: with |b3| <= 3 none of y's two roundings would ever round, and a kernel that skipped one would pass.  So every second
    channel of b3 is an integer |b3| <= 400: there conv3 + b3 reaches 2^8 .. 2^9, where bf16 keeps even integers only, both roundings
    (ties included) act, and y's sign is the bias's; the other channels keep |b3| <= 3, where the residual decides the ReLU.  GEMM 2
    then sums 512 integers |y| < 2^9 times {-1, 0, 1}: below 2^18, and t1's rounding acts on integers up to 2^14."""
    from tests.conv_checks import Data, check

    n, h, w = shape
    d = Data(True, 7000 + ALL_SHAPES.index(shape), DEV)
    t2, res = d.act((n, h, w, 128)), d.act((n, h, w, 512), hi=8)
    w3l, w1l = d.weight((512, 128), 128), d.weight((128, 512), 512)
    b3, b1 = d.bias(512, 512), d.bias(128, 128)
    b3[1::2] = torch.randint(-400, 401, (256,), generator=d.g, device=DEV).float()
    y_ref, t1_ref = cc.reference_pw_chain(t2, res, w3l, b3, w1l, b1, exact=True)
    rounded = (cc.conv_sum(t2, w3l[:, None, None, :], cc._plain(n, h, w, 128, 1, 1, 0, 512)) + b3.double()).abs() > 256
    assert 0.1 < float(rounded.double().mean()) < 0.9 and 0.2 < float((y_ref == 0).double().mean()) < 0.8
    y, t1 = _sentinel_call(t2, res, cc.pack_weight(w3l[:, None, None, :], 0, 128, 512), b3, cc.pack_weight(w1l[:, None, None, :], 0, 512, 128), b1)
    check(y, y_ref, True)
    check(t1, t1_ref, True)
    print(f"{shape}: y and t1 exact; {100 * float(rounded.double().mean()):.0f} % of conv3 + b3 past 2^8, {100 * float((y_ref == 0).double().mean()):.0f} % of y zero")


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_IDS)
def test_gaussian_regime_y_and_t1_within_the_float64_contract(shape):
    """y within conv3's bound of float64, t1 within conv1's bound of float64 on the DEVICE's own y (one conv's bound each)"""
    from tests.conv_checks import check

    pc3, pc1, pk = _packs()
    t2, res, y_two, t1_two = _case(shape)
    y, t1 = _sentinel_call(t2, res, pk.w3, pk.b3, pk.w1, pk.b1)
    assert torch.equal(y, y_two) and torch.equal(t1, t1_two)     # and the two md_conv2d launches, bit for bit, on the two new shapes too
    n, h, w = shape
    ry = check(y, cc.conv_stage(t2, 0.0, pc3.w.view(512, 1, 1, 128), pc3.bias, cc._plain(n, h, w, 128, 1, 1, 0, 512), 1, res=res.double()), False)
    rt = check(t1, cc.conv_stage(y.double(), 0.0, pc1.w.view(128, 1, 1, 512), pc1.bias, cc._plain(n, h, w, 512, 1, 1, 0, 128), 1), False)
    print(f"{shape}: worst err / bound: y {ry:.4f}, t1 on the device's y {rt:.4f}")


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
