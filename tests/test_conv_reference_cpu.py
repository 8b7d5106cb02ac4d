"""The float64 conv reference of tests/conv_contract.py (what tests/test_conv_production_gpu.py holds every production call to), checked
on the CPU against float64 F.conv2d / F.conv_transpose2d composed by hand, one addressing feature of md_conv2d_attrs at a time.  A
reference that misread the header would otherwise agree with a kernel that misreads it the same way.

Data are small integers (weights {-1, 0, 1}), so every value is exact in float64 and in bf16 where the composition rounds through
torch's own fp32 -> bf16 cast: the comparisons are exact."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_contract as cc

BF = torch.bfloat16


def ints(shape, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-hi, hi + 1, shape, generator=g).double()


def rnd(v):
    """bf16 rounding by torch's cast (fp32-exact values)"""
    return v.float().to(BF).double()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def torch_conv(x, wl, stride=1, pad=(0, 0, 0, 0)):
    """float64 F.conv2d of NHWC x with a [cout, kh, kw, cin] weight after F.pad(pad = (left, right, top, bottom)) -> NHWC"""
    return nhwc(F.conv2d(F.pad(nchw(x), pad), wl.permute(0, 3, 1, 2), stride=stride))


def ref(x, wl, b, r, shapes, a):
    return cc.reference_conv2d(x, wl, b, r, shapes, a)


@pytest.mark.parametrize("kh,stride,pad,cin,korder", [(1, 1, 0, 64, 0), (3, 1, 1, 64, 0), (3, 1, 1, 128, 1), (3, 2, 1, 64, 1),
                                                       (7, 2, 3, 8, 0), (1, 2, 0, 32, 0)])
def test_plain_conv_and_both_k_orders(kh, stride, pad, cin, korder):
    x, wl, b = ints((2, 11, 13, cin), 2, 1), ints((24, kh, kh, cin), 1, 2), ints((24,), 3, 3)
    ho, wo = (11 + 2 * pad - kh) // stride + 1, (13 + 2 * pad - kh) // stride + 1
    kpad = (kh * kh * cin + 63) // 64 * 64
    shapes = [list(x.shape), [32, kpad], [32], None, [2, ho, wo, 24]]
    a = cc.conv_attrs(kh, stride, pad, relu=0, korder=korder)
    want = torch_conv(x, wl, stride, (pad,) * 4) + b
    assert torch.equal(ref(x, wl, b, None, shapes, a), rnd(want))
    # the packed operand: element (c, k) of the header's K order
    wp = cc.pack_weight(wl, korder, kpad, 32)
    assert wp.shape == (32, kpad) and not wp[24:].any() and not wp[:, kh * kh * cin:].any()
    for c, i, j, ci in ((0, 0, 0, 0), (5, kh - 1, kh // 2, cin - 1), (23, kh // 2, kh - 1, 17 % cin), (7, 0, kh - 1, cin // 2 + 3)):
        k = (ci // 64 * kh * kh + i * kh + j) * 64 + ci % 64 if korder else (i * kh + j) * cin + ci
        assert wp[c, k] == wl[c, i, j, ci]


def test_activations_and_rounding():
    x, wl, b = ints((2, 9, 10, 64), 2, 4), ints((40, 3, 3, 64), 1, 5), ints((40,), 3, 6)
    shapes = [list(x.shape), [64, 576], [64], None, [2, 9, 10, 40]]
    for relu in (0, 1):
        want = torch_conv(x, wl, 1, (1,) * 4) + b
        want = rnd(F.relu(want) if relu else want)
        assert torch.equal(ref(x, wl, b, None, shapes, cc.conv_attrs(3, 1, 1, relu=relu)), want)
    # SiLU: float64 silu rounded to bf16 once
    wq = wl / 8
    want = torch_conv(x, wq, 1, (1,) * 4) + b
    got = ref(x, wq, b, None, shapes, cc.conv_attrs(3, 1, 1, relu=2))
    assert torch.equal(got, cc.bf16_rne(want * torch.sigmoid(want)))
    # bf16_rne: one rounding, ties to even, against torch's cast where fp32 holds the value exactly
    v = torch.tensor([1 + 2 ** -8, 1 + 3 * 2 ** -8, -(1 + 2 ** -8), 257.0, 259.0, 2 ** -130 * 1.5, 0.0, 3 * 2 ** -10, 1e30], dtype=torch.float64)
    assert torch.equal(cc.bf16_rne(v), rnd(v))
    assert cc.bf16_rne(torch.tensor([1 + 2 ** -8 + 2 ** -40], dtype=torch.float64))[0] == 1 + 2 ** -7   # just above the tie: up (fp32 would tie to 1)


def test_asymmetric_padding_and_sub_window():
    x, wl, b = ints((2, 12, 15, 64), 2, 7), ints((16, 3, 3, 64), 1, 8), ints((16,), 3, 9)
    for pt, pl, s, sh, sw in ((0, 1, 1, 11, 13), (1, 0, 2, 6, 7), (2, 0, 1, 12, 9), (0, 0, 2, 5, 7)):
        a = cc.conv_attrs(3, s, 0, adv=1, pad_top=pt, pad_left=pl, sub_h=sh, sub_w=sw, out_stride=1, cout=16)
        want = torch_conv(x, wl, s, (pl, 8, pt, 8))[:, :sh, :sw] + b
        assert torch.equal(ref(x, wl, b, None, [list(x.shape), [16, 576], [16], None, [2, sh, sw, 16]], a), rnd(want)), (pt, pl, s)


def test_subpixel_parities_compose_a_transposed_conv():
    """CenterNet's Conv2dTranspose(k=4, s=2, p=1) as four k = 2 convs, output parity (py, px) <- taps (3 - py - 2 t) of the kernel at
    input row ho + py - 1 + t; Mask R-CNN's k = s = 2 deconv as four 1x1 convs.  Every out_off parity of out_stride 2."""
    x, b = ints((2, 7, 9, 64), 2, 10), ints((32,), 3, 11)
    wt = ints((64, 32, 4, 4), 1, 12)                                   # ConvTranspose2d weight [cin, cout, kh, kw]
    want = nhwc(F.conv_transpose2d(nchw(x), wt, stride=2, padding=1)) + b
    y = torch.full((2, 14, 18, 32), float("nan"), dtype=torch.float64)
    for py in (0, 1):
        for px in (0, 1):
            taps_y, taps_x = [3 - py, 1 - py], [3 - px, 1 - px]
            wl = wt[:, :, taps_y][:, :, :, taps_x].permute(1, 2, 3, 0)   # [cout, 2, 2, cin]
            a = cc.conv_attrs(2, 1, 0, adv=1, pad_top=1 - py, pad_left=1 - px, sub_h=7, sub_w=9, out_stride=2, out_off_y=py,
                              out_off_x=px, cout=32)
            part = ref(x, wl, b, None, [list(x.shape), [32, 256], [32], None, list(y.shape)], a)
            written = ~part.isnan()
            assert int(written.sum()) == 2 * 7 * 9 * 32 and not (written & ~y.isnan()).any()
            y[written] = part[written]
    assert torch.equal(y, rnd(want))
    wt2 = ints((64, 32, 2, 2), 1, 13)
    want = nhwc(F.conv_transpose2d(nchw(x), wt2, stride=2)) + b
    y = torch.full((2, 14, 18, 32), float("nan"), dtype=torch.float64)
    for py in (0, 1):
        for px in (0, 1):
            a = cc.conv_attrs(1, 1, 0, adv=1, sub_h=7, sub_w=9, out_stride=2, out_off_y=py, out_off_x=px, cout=32)
            part = ref(x, wt2[:, :, py, px].t()[:, None, None, :], b, None, [list(x.shape), [32, 64], [32], None, list(y.shape)], a)
            written = ~part.isnan()
            y[written] = part[written]
    assert torch.equal(y, rnd(want))


def test_channel_slices_in_and_out():
    """x_c_off / x_cin: the conv reads a channel range of a wider x; c_off: it writes a channel range of a wider y"""
    x, wl, b = ints((2, 8, 9, 192), 2, 14), ints((40, 3, 3, 64), 1, 15), ints((40,), 3, 16)
    a = cc.conv_attrs(3, 1, 1, relu=1, x_c_off=64, x_cin=64, korder=1)
    want = F.relu(torch_conv(x[..., 64:128], wl, 1, (1,) * 4) + b)
    assert torch.equal(ref(x, wl, b, None, [list(x.shape), [64, 576], [64], None, [2, 8, 9, 40]], a), rnd(want))
    a = cc.conv_attrs(3, 1, 1, relu=1, x_c_off=128, x_cin=64, adv=1, pad_top=1, pad_left=1, sub_h=8, sub_w=9, out_stride=1,
                      c_off=56, cout=40)
    y = ref(x, wl, b, None, [list(x.shape), [64, 576], [64], None, [2, 8, 9, 128]], a)
    want = F.relu(torch_conv(x[..., 128:], wl, 1, (1,) * 4) + b)
    assert torch.equal(y[..., 56:96], rnd(want)) and y[..., :56].isnan().all() and y[..., 96:].isnan().all()


def test_residual_slice_and_residual_rounding():
    """res_slice / res_c_off (the C2f bottleneck: x + silu(conv(x)) out of one concat buffer): t = bf16(act(conv + b)), y = bf16(t + r)"""
    x, wl, b = ints((2, 8, 9, 128), 2, 17), ints((64, 3, 3, 64), 1, 18), ints((64,), 3, 19)
    r = ints((2, 8, 9, 192), 8, 20)
    for relu in (1, 2, 0):
        a = cc.conv_attrs(3, 1, 0, relu=relu, korder=1, x_c_off=64, x_cin=64, adv=1, pad_top=1, pad_left=1, sub_h=8, sub_w=9,
                          out_stride=1, c_off=64, cout=64, res_slice=1, res_c_off=128)
        wq = wl / 8 if relu == 2 else wl
        pre = torch_conv(x[..., 64:], wq, 1, (1,) * 4) + b
        t = cc.bf16_rne(pre * torch.sigmoid(pre)) if relu == 2 else rnd(pre)
        want = rnd(t + r[..., 128:])
        want = F.relu(want) if relu == 1 else want
        y = ref(x, wq, b, r, [list(x.shape), [64, 576], [64], list(r.shape), [2, 8, 9, 192]], a)
        assert torch.equal(y[..., 64:128], want), relu
        if relu == 2:   # one rounding after the add instead of two: the exact regime tells them apart
            assert not torch.equal(y[..., 64:128], cc.bf16_rne(pre * torch.sigmoid(pre) + r[..., 128:]))
        assert y[..., :64].isnan().all() and y[..., 128:].isnan().all()


@pytest.mark.parametrize("ho,wo", [(10, 12), (9, 11)])
def test_upsampled_residual(ho, wo):
    """res_upsample: the residual [N, ceil(Ho/2), ceil(Wo/2), Cout] added with nearest 2x upsampling (FPN top-down add)"""
    x, wl, b = ints((2, ho, wo, 64), 2, 21), ints((32, 1, 1, 64), 1, 22), ints((32,), 3, 23)
    r = ints((2, (ho + 1) // 2, (wo + 1) // 2, 32), 8, 24)
    up = nhwc(F.interpolate(nchw(r), scale_factor=2, mode="nearest"))[:, :ho, :wo]
    want = rnd(rnd(torch_conv(x, wl) + b) + up)
    a = cc.conv_attrs(1, res_upsample=1)
    assert torch.equal(ref(x, wl, b, r, [list(x.shape), [32, 64], [32], list(r.shape), [2, ho, wo, 32]], a), want)


def test_head_form():
    """md_conv2d_head: y2 = bf16(b2 + w2[:16] . bf16(relu(conv3x3(x) + b))), as the GPU test composes it"""
    x, wl, b = ints((2, 9, 11, 64), 2, 25), ints((256, 3, 3, 64), 1, 26), ints((256,), 3, 27)
    w2, b2 = ints((16, 256), 1, 28), ints((16,), 3, 29)
    shapes = [list(x.shape), [256, 576], [256], [32, 256], [32], [2, 9, 11, 16]]
    g = cc.conv_geometry(shapes, cc.conv_attrs(3, 1, 1, relu=1, korder=1))
    assert (g.cout, g.sub_h, g.sub_w, g.k) == (256, 9, 11, 576)
    got = cc.reference_head(x, wl, b, w2, b2, g)
    mid = rnd(F.relu(torch_conv(x, wl, 1, (1,) * 4) + b))
    want = rnd(torch_conv(mid, w2[:, None, None, :]) + b2)
    assert torch.equal(got, want)


def test_dual_form_with_stride_two():
    """md_conv1x1_dual: bf16(relu(w . [x_a ; x_b[::2, ::2]] + b)) = the block's conv3 + strided downsample + add, summed once"""
    xa, xb = ints((2, 5, 6, 64), 2, 30), ints((2, 10, 11, 128), 2, 31)
    w, b = ints((96, 192), 1, 32), ints((96,), 3, 33)
    got = cc.reference_dual(xa, xb, w, b, 2, 1)
    want = torch_conv(xa, w[:, None, None, :64]) + torch_conv(xb, w[:, None, None, 64:], stride=2) + b
    assert torch.equal(got, rnd(F.relu(want)))
    assert torch.equal(cc.dual_sum(xa, xb, -w, 2, absolute=True), cc.dual_sum(xa.abs(), xb.abs(), w.abs(), 2))


def test_gaussian_bound_holds_for_an_fp32_computation():
    """the Gaussian-regime bound against an actual fp32 (sequential) accumulation with the same rounding points"""
    g = torch.Generator().manual_seed(34)
    x = torch.randn((1, 6, 7, 64), generator=g).to(BF).double()
    wl = (torch.randn((16, 3, 3, 64), generator=g) / 24).to(BF).double()
    b, r = torch.randn((16,), generator=g).double(), torch.randn((1, 6, 7, 16), generator=g).to(BF).double()
    geo = cc.conv_geometry([list(x.shape), [16, 576], [16], None, [1, 6, 7, 16]], cc.conv_attrs(3, 1, 1))
    pre = cc.conv_sum(x, wl, geo) + b
    absum = cc.conv_sum(x, wl, geo, absolute=True) + b.abs()
    acc = torch.zeros((1, 6, 7, 16), dtype=torch.float32)     # fp32, one tap-channel at a time
    xp = F.pad(x, (0, 0, 1, 1, 1, 1)).float()
    for i in range(3):
        for j in range(3):
            for ci in range(64):
                acc = acc + xp[:, i:i + 6, j:j + 7, ci:ci + 1] * wl[:, i, j, ci].float()
    acc = acc + b.float()
    c = cc.accumulation_c(geo.k + 1)
    for relu in (0, 1, 2):
        t = acc * torch.sigmoid(acc) if relu == 2 else acc
        y = rnd(F.relu(rnd(t) + r) if relu == 1 else rnd(t) + r)
        want, bound = cc.gaussian_bound(pre, absum, c, relu, r.double())
        assert ((y - want).abs() <= bound).all(), relu


def test_stem_pool_stem_conv_and_bottleneck():
    """md_stem_pool (conv 7x7/s2/p3 + ReLU -> bf16 -> MaxPool 3x3/s2/p1), md_stem_conv (6x6/s2/p2 and 3x3/s2/p1 + SiLU) on the stem
    layout, and md_bottleneck in its three residual forms, against F.conv2d / F.max_pool2d; plus the packed stem weight layouts"""
    img, b64 = ints((2, 16, 64, 3), 2, 35), ints((64,), 3, 36)
    x4 = torch.zeros((2, 32, 80, 4), dtype=torch.float64)
    x4[:, 7:23, 7:71, :3] = img
    wl = ints((64, 7, 7, 3), 1, 37)
    want = rnd(F.relu(torch_conv(img, wl, 2, (3,) * 4) + b64))
    assert torch.equal(cc.reference_stem_pool(x4, wl, b64), nhwc(F.max_pool2d(nchw(want), 3, 2, 1)))
    wp = cc.pack_stem_pool(wl).reshape(64, 7, 8, 4)
    assert torch.equal(wp[:, :, :7, :3], wl) and not wp[:, :, 7].any() and not wp[..., 3].any()
    for k, p in ((6, 2), (3, 1)):
        w = ints((32, k, k, 3), 1, 38 + k) / 4
        pre = torch_conv(img, w, 2, (p,) * 4) + b64[:32]
        assert torch.equal(cc.reference_stem_conv(x4, w, b64[:32], 2), pre)
        wp = cc.pack_stem_conv(w).reshape(32, k, 8 if k == 6 else 4, 4)
        x0 = 1 if k == 6 else 0
        assert torch.equal(wp[:, :, x0:x0 + k, :3], w) and not wp[..., 3].any() and wp.abs().sum() == w.abs().sum()
    x = ints((2, 6, 7, 64), 1, 44)
    w1, w2, w3, wd = ints((64, 64), 1, 45), ints((64, 3, 3, 64), 1, 46), ints((256, 64), 1, 47), ints((256, 64), 1, 48)
    b1, b2, b3, bd = ints((64,), 3, 49), ints((64,), 3, 50), ints((256,), 3, 51), ints((256,), 3, 52)
    t1 = rnd(F.relu(torch_conv(x, w1[:, None, None, :]) + b1))
    t2 = rnd(F.relu(torch_conv(t1, w2, 1, (1,) * 4) + b2))
    t3 = rnd(torch_conv(t2, w3[:, None, None, :]) + b3)
    r = ints((2, 6, 7, 256), 1, 53)
    for res, wd_, bd_, resid in ((r, None, None, r), (None, wd, bd, rnd(torch_conv(x, wd[:, None, None, :]) + bd))):
        assert torch.equal(cc.reference_bottleneck(x, w1, b1, w2, b2, w3, b3, res, wd_, bd_), F.relu(rnd(t3 + resid)))
    x256 = ints((2, 6, 7, 256), 1, 54)
    w1 = ints((64, 256), 1, 55)
    t1 = rnd(F.relu(torch_conv(x256, w1[:, None, None, :]) + b1))
    t3 = rnd(torch_conv(rnd(F.relu(torch_conv(t1, w2, 1, (1,) * 4) + b2)), w3[:, None, None, :]) + b3)
    assert torch.equal(cc.reference_bottleneck(x256, w1, b1, w2, b2, w3, b3), F.relu(rnd(t3 + x256)))


def test_gaussian_chain_bound_holds_for_an_fp32_bottleneck():
    """the propagated bound of a chain (md_bottleneck's, the head's) against the chain computed in fp32 with bf16 rounding points"""
    g = torch.Generator().manual_seed(56)
    x = torch.randn((1, 5, 6, 64), generator=g).to(BF).double()
    w1, w2, w3 = ((torch.randn(s, generator=g) / k ** 0.5).to(BF).double() for s, k in (((64, 64), 64), ((64, 3, 3, 64), 576), ((256, 64), 64)))
    b1, b2, b3 = (torch.randn((c,), generator=g).double() for c in (64, 64, 256))
    f = lambda t, w, p=0: nhwc(F.conv2d(F.pad(nchw(t).float(), (p,) * 4), w.permute(0, 3, 1, 2).float())).double()
    t1 = rnd(F.relu(f(x, w1[:, None, None, :]) + b1))
    t2 = rnd(F.relu(f(t1, w2, 1) + b2))
    y = F.relu(rnd(rnd(f(t2, w3[:, None, None, :]) + b3) + x.repeat(1, 1, 1, 4)))
    want, bound = cc.reference_bottleneck(x, w1, b1, w2, b2, w3, b3, x.repeat(1, 1, 1, 4), exact=False)
    assert ((y - want).abs() <= bound).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# md_conv2d_grouped: the reference and the packer of conv_contract, and how much the contract's two regimes see
# ---------------------------------------------------------------------------------------------------------------------------------
def torch_grouped(x, wls, biases, k, x_c_off):
    """float64 F.conv2d(groups=G) on the groups' slices of NHWC x, every group's weight padded to 16 rows -> per group [n, H, W, cout_g]"""
    G = len(wls)
    wf, bf = torch.zeros((16 * G, 64, k, k), dtype=torch.float64), torch.zeros((16 * G,), dtype=torch.float64)
    for g, (wl, b) in enumerate(zip(wls, biases)):
        wf[16 * g:16 * g + wl.shape[0]] = wl.permute(0, 3, 1, 2)
        bf[16 * g:16 * g + wl.shape[0]] = b
    y = nhwc(F.conv2d(nchw(x[..., x_c_off:x_c_off + 64 * G]), wf, bf, padding=k // 2, groups=G))
    return [y[..., 16 * g:16 * g + wl.shape[0]] for g, wl in enumerate(wls)]


@pytest.mark.parametrize("k", [1, 3])
def test_grouped_reference_against_torch(k):
    """x_c_off != 0 on a tensor with trailing channels, out-of-order y_off with gaps, every written element and only those"""
    couts, y_offs, cy = [3, 1, 2, 16, 5], [40, 3, 37, 8, 27], 48
    x = ints((2, 7, 9, 8 + 320 + 16), 2, 60)
    wls = [ints((c, k, k, 64), 1, 61 + g) for g, c in enumerate(couts)]
    biases = [ints((c,), 3, 70 + g) for g, c in enumerate(couts)]
    for relu in (0, 1):
        a = cc.grouped_attrs(k, couts, y_offs, relu=relu, x_c_off=8)
        geos = cc.grouped_geometries(x.shape, a, (2, 7, 9, cy))
        assert [(g.x_c_off, g.c_off, g.cout, g.cin, g.k) for g in geos] == [(8 + 64 * i, y_offs[i], couts[i], 64, 64 * k * k) for i in range(5)]
        y = cc.reference_grouped(x, wls, biases, a, (2, 7, 9, cy))
        written = torch.zeros(cy, dtype=torch.bool)
        for g, want in enumerate(torch_grouped(x, wls, biases, k, 8)):
            written[y_offs[g]:y_offs[g] + couts[g]] = True
            assert torch.equal(y[..., y_offs[g]:y_offs[g] + couts[g]], rnd(F.relu(want) if relu else want)), (relu, g)
        assert y[..., ~written].isnan().all() and not y[..., written].isnan().any()
        # the Gaussian-regime form: the same values before the rounding, a bound on exactly the written elements
        v, bound = cc.reference_grouped(x, wls, biases, a, (2, 7, 9, cy), exact=False)
        assert torch.equal(v.isnan(), y.isnan()) and torch.equal(bound.isnan(), y.isnan()) and bool((bound[..., written] > 0).all())
        assert torch.equal(rnd(v[..., written]), y[..., written])


def test_grouped_packers_agree():
    """conv_contract.pack_grouped, written from the header, and nn_ops.pack_conv2d_grouped give one operand for BN-free convs"""
    from minddet_amd import nn_ops

    for k in (1, 3):
        couts = [2, 16, 1, 3]
        wls = [ints((c, k, k, 64), 1, 80 + g) for g, c in enumerate(couts)]
        biases = [ints((c,), 3, 90 + g) for g, c in enumerate(couts)]
        w, b, rows = cc.pack_grouped([wl.to(BF) for wl in wls], biases)
        pk = nn_ops.pack_conv2d_grouped([(wl.permute(0, 3, 1, 2).float(), bb.float(), None) for wl, bb in zip(wls, biases)])
        assert rows == pk.w_rows == [0, 2, 18, 19] and pk.couts == couts and pk.k == k
        assert w.dtype == pk.w.dtype == BF and torch.equal(w, pk.w) and b.dtype == pk.bias.dtype and torch.equal(b, pk.bias)
        # element (row, K) of the header, and rows of one's own choosing
        assert w[2 + 7, (k * k - 1) * 64 + 5] == wls[1][7, k - 1, k - 1, 5] and w[19 + 2, (k // 2 * k) * 64 + 63] == wls[3][2, k // 2, 0, 63]
        w2, b2, rows2 = cc.pack_grouped(wls, biases, w_rows=[20, 0, 19, 16], rows=24, fill=7.0)
        assert rows2 == [20, 0, 19, 16] and torch.equal(w2[0:16], w[2:18].double()) and torch.equal(w2[20:22], w[0:2].double())
        assert bool((w2[22:] == 7).all()) and bool((b2[22:] == 7).all()) and torch.equal(b2[16:19], b[19:22])


def _simulated_kernel(x, wls, biases, a, y_shape, defect=None):
    """md_conv2d_grouped as a correct kernel computes it -- fp32 F.conv2d per group, bias, ReLU, one rounding to bf16 -- into a
    NaN-filled y; defect: 'swap' two input channels within every group, 'tap' drop one tap, 'column' zero image column 32 of x"""
    y = torch.full(y_shape, float("nan"), dtype=BF)
    k = a["k"]
    xf = x.float()
    if defect == "column":
        xf = xf.clone()
        xf[:, :, 32] = 0
    for g, (wl, b) in enumerate(zip(wls, biases)):
        c0 = a["x_c_off"] + 64 * g
        xs = xf[..., c0:c0 + 64]
        w = wl.float()
        if defect == "swap":
            xs = xs[..., [0, 1, 2, 3, 4, 9, 6, 7, 8, 5] + list(range(10, 64))]
        if defect == "tap":
            w = w.clone()
            w[:, 0, k - 1] = 0
        v = nhwc(F.conv2d(nchw(xs), w.permute(0, 3, 1, 2), b.float(), padding=k // 2))
        y[..., a["y_off"][g]:a["y_off"][g] + a["cout"][g]] = (F.relu(v) if a["relu"] else v).to(BF)
    return y


def test_grouped_contract_passes_a_correct_kernel_and_sees_three_defects():
    """On the draws the GPU test makes (conv_checks.grouped_operands of the ragged case, on the CPU generator): an fp32 computation with
    one bf16 rounding is bit-equal to the reference in the exact regime and within the bound everywhere in the Gaussian regime; two
    swapped input channels, a dropped tap and a zeroed image column at the tile boundary each break both."""
    from tests.conv_checks import grouped_operands

    for exact in (True, False):
        x, wls, biases, a, y_shape = grouped_operands("ragged", exact, "cpu")
        ref = cc.reference_grouped(x, wls, biases, a, y_shape, exact=exact)
        y, bound = (ref, None) if exact else ref
        written = ~y.isnan()

        def wrong(defect):
            """fraction of the written elements that miss the contract"""
            got = _simulated_kernel(x, wls, biases, a, y_shape, defect).double()
            assert torch.equal(got.isnan(), ~written)
            bad = got[written] != y[written] if exact else (got[written] - y[written]).abs() > bound[written]
            return float(bad.double().mean())

        assert wrong(None) == 0.0, exact
        for defect, least in (("swap", 0.5), ("tap", 0.5), ("column", 0.02)):
            f = wrong(defect)
            print(f"exact={exact} {defect}: {100 * f:.1f} % of the elements miss the contract")
            assert f >= least, (exact, defect, f)
        if not exact:
            got = _simulated_kernel(x, wls, biases, a, y_shape).double()
            print(f"correct kernel, Gaussian regime: worst err / bound {float(((got[written] - y[written]).abs() / bound[written]).max()):.3f}")
