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


# ---------------------------------------------------------------------------------------------------------------------------------
# md_c3_pair and md_pw_chain: the references of conv_contract, the exact draw's conditions, and what the two regimes see
# ---------------------------------------------------------------------------------------------------------------------------------
def _c3_small_cases():
    from tests.test_c3pair_gpu import SMALL

    return SMALL


def _c3_case(name):
    return next(c for c in _c3_small_cases() if c[0] == name)


def _c3_draw(case, exact):
    from tests.conv_checks import c3_pair_operands

    return c3_pair_operands(case, exact, "cpu")


def silu_by_hand(pre):
    """float64 SiLU through torch.sigmoid, rounded to bf16 once"""
    return cc.bf16_rne(pre * torch.sigmoid(pre))


@pytest.mark.parametrize("name", ["c32_offsets_pass_through", "c32_ragged", "c128_offsets_no_second_half", "c128_ragged", "c64_offsets"])
def test_c3_pair_reference_against_torch(name):
    """reference_c3_pair against F.conv2d composed by hand with a rounding at each of the header's rounding points: C = 32 (K order 0)
    and C = 128 (K order 1), with and without the shortcut, with x_c_off != 0 (NaN in every channel of x outside the slice); and the
    packed operands element by element against the header's K orders"""
    name, n, h, w, c, shortcut, passt, xc, xo = _c3_case(name)[:9]
    x, w1l, b1, w2l, b2 = (v.double() for v in _c3_draw(_c3_case(name), True))
    assert x[..., :xo].isnan().all() and x[..., xo + (2 * c if passt else c):].isnan().all() and not x[..., xo:xo + c].isnan().any()
    xs = x[..., xo:xo + c]
    pre1 = torch_conv(xs, w1l[:, None, None, :]) + b1
    t_want = silu_by_hand(pre1)
    pre2_want = torch_conv(t_want, w2l, 1, (1,) * 4) + b2                     # F.conv2d's zero padding pads t
    for sc in (False, True):
        t, pre2, res = cc.reference_c3_pair(x, w1l, b1, w2l, b2, xo, sc, exact=True)
        assert torch.equal(t, t_want) and torch.equal(pre2, pre2_want)        # multiples of 2^-13 below 2^6: exact in float64
        assert (res is None) if not sc else torch.equal(res, xs)
        u = silu_by_hand(pre2)
        assert torch.equal(cc.epilogue(pre2, 2, res), rnd(u + xs) if sc else u)
        # the Gaussian form: the unrounded float64 chain and a positive bound
        v, bound = cc.reference_c3_pair(x, w1l, b1, w2l, b2, xo, sc, exact=False)
        p1 = pre1 * torch.sigmoid(pre1)
        p2 = torch_conv(p1, w2l, 1, (1,) * 4) + b2
        assert torch.allclose(v, p2 * torch.sigmoid(p2) + (xs if sc else 0), rtol=1e-12, atol=1e-12) and bool((bound > 0).all())
    w1, w2 = cc.c3_pair_weights(w1l, w2l)
    assert tuple(w1.shape) == (c, (c + 63) // 64 * 64) and tuple(w2.shape) == (c, (9 * c + 63) // 64 * 64)
    assert torch.equal(w1[:, :c], w1l) and not w1[:, c:].any() and not w2[:, 9 * c:].any()
    for co, i, j, ci in ((0, 0, 0, 0), (c - 1, 2, 2, c - 1), (5, 1, 2, c // 2 + 3), (17, 2, 0, 31), (c // 2, 0, 1, c - 30)):
        tap = 3 * i + j
        k = tap * 32 + ci if c == 32 else (ci // 64) * 576 + tap * 64 + ci % 64
        assert w2[co, k] == w2l[co, i, j, ci]


def test_c3_pair_exact_draw_keeps_the_chain_exact_for_every_case():
    """conditions (a) to (d) of reference_c3_pair (asserted inside it) on the very draws the GPU test uses, every small case: no
    stage-1 value near a rounding midpoint, both stages exact in fp32, the either-neighbour share of stage 2 at most 2e-3"""
    for case in _c3_small_cases():
        x, w1l, b1, w2l, b2 = _c3_draw(case, True)
        t, pre2, _ = cc.reference_c3_pair(x, w1l, b1, w2l, b2, case[8], case[5], exact=True)
        g2 = cc._plain(case[1], case[2], case[3], case[4], 3, 1, 1, case[4])
        unit = float(cc.bf16_quantum(t[t != 0]).min()) * cc.grid(w2l)
        bits = cc.fp32_exact_bits(cc.conv_sum(t, w2l, g2, absolute=True) + b2.double().abs(), unit)
        share = float(cc.silu_rounding(pre2)[2].double().mean())
        print(f"{case[0]}: smallest quantum of t 2^{torch.log2(cc.bf16_quantum(t[t != 0]).min()).item():.0f}, stage 2 needs {bits:.1f} bits, "
              f"pre2 in [{pre2.min().item():.1f}, {pre2.max().item():.1f}] (std {pre2.std().item():.1f}), either-neighbour share {share:.2e}")
        assert bits < 24 and share <= cc.NEAR_CAP == 2e-3


def test_c3_pair_reference_refuses_a_draw_that_is_not_exact():
    """the asserted conditions bite: a stage-1 value at a rounding midpoint of SiLU, and stage-2 weights on too fine a grid"""
    case = _c3_case("c32_one_tile_exact")
    x, w1l, b1, w2l, b2 = (v.double() for v in _c3_draw(case, True))
    with pytest.raises(AssertionError, match=r"\(b\)"):
        cc.reference_c3_pair(x, w1l, b1, w2l * (1 + 2.0 ** -7) * 2.0 ** -12, b2, 0, True)
    # a bias on the 2^-20 grid whose SiLU lies at the bf16 midpoint 1 + 2^-8 (bisection on v), with w1 scaled to 2^-20 so that
    # stage 1 stays exact in fp32: wherever a pixel's six inputs are all zero the pre-activation is that bias
    lo, hi = torch.tensor(1.0, dtype=torch.float64), torch.tensor(2.0, dtype=torch.float64)
    for _ in range(60):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if cc.silu64(mid) < 1 + 2.0 ** -8 else (lo, mid)
    v = torch.round(lo * 2.0 ** 20) * 2.0 ** -20
    assert bool(cc.silu_rounding(v)[2])
    with pytest.raises(AssertionError, match=r"\(a\)"):
        cc.reference_c3_pair(x, w1l * 2.0 ** -19, torch.full_like(b1, float(v)), w2l, b2, 0, True)


def test_pw_chain_reference_against_torch():
    """reference_pw_chain against F.conv2d composed by hand: y = relu(rnd(rnd(conv3 + b3) + res)), t1 = rnd(relu(conv1(y) + b1)), a
    residual of both signs, biases wide enough that both of y's roundings round"""
    t2, res = ints((2, 5, 7, 128), 2, 100), ints((2, 5, 7, 512), 8, 101)
    w3, w1 = ints((512, 128), 1, 102), ints((128, 512), 1, 103)
    b3, b1 = ints((512,), 400, 104), ints((128,), 3, 105)
    v = rnd(torch_conv(t2, w3[:, None, None, :]) + b3)
    y_want = F.relu(rnd(v + res))
    t1_want = rnd(F.relu(torch_conv(y_want, w1[:, None, None, :]) + b1))
    y, t1 = cc.reference_pw_chain(t2, res, w3, b3, w1, b1)
    assert torch.equal(y, y_want) and torch.equal(t1, t1_want)
    assert bool((res > 0).any()) and bool((res < 0).any()) and 0.2 < float((y == 0).double().mean()) < 0.8
    assert not torch.equal(y, F.relu(rnd(torch_conv(t2, w3[:, None, None, :]) + b3 + res)))     # the two roundings are seen
    (yv, ey), (tv, et) = cc.reference_pw_chain(t2, res, w3, b3, w1, b1, exact=False)
    assert torch.equal(yv, F.relu(torch_conv(t2, w3[:, None, None, :]) + b3 + res)) and bool((ey > 0).all()) and bool((et > 0).all())
    assert torch.equal(tv, F.relu(torch_conv(yv, w1[:, None, None, :]) + b1))


def _f32conv(t, w, p=0):
    """fp32 F.conv2d of NHWC t (float64 values that fp32 holds) with a [cout, kh, kw, cin] weight, zero padding p -> float64"""
    return nhwc(F.conv2d(F.pad(nchw(t).float(), (p,) * 4), w.permute(0, 3, 1, 2).float())).double()


def test_gaussian_chain_bound_holds_for_an_fp32_c3_pair_and_pw_chain():
    """the propagated bounds of reference_c3_pair and reference_pw_chain against the chains computed in fp32 with bf16 rounding points"""
    g = torch.Generator().manual_seed(110)
    silu32 = lambda v: F.silu(v.float()).double()
    for c, sc in ((32, True), (128, True), (64, False)):
        x = torch.randn((1, 6, 7, c + 16), generator=g).to(BF).double()
        w1, w2 = ((torch.randn(s, generator=g) / k ** 0.5).to(BF).double() for s, k in (((c, c), c), ((c, 3, 3, c), 9 * c)))
        b1, b2 = torch.randn((c,), generator=g).float(), torch.randn((c,), generator=g).float()
        xs = x[..., 8:8 + c]
        t = rnd(silu32(_f32conv(xs, w1[:, None, None, :]) + b1))
        u = rnd(silu32(_f32conv(t, w2, 1) + b2))
        y = rnd(u + xs) if sc else u
        want, bound = cc.reference_c3_pair(x, w1, b1, w2, b2, 8, sc, exact=False)
        assert ((y - want).abs() <= bound).all(), c
    t2, res = torch.randn((1, 5, 6, 128), generator=g).to(BF).double(), torch.randn((1, 5, 6, 512), generator=g).to(BF).double()
    w3, w1 = ((torch.randn(s, generator=g) / s[1] ** 0.5).to(BF).double() for s in ((512, 128), (128, 512)))
    b3, b1 = torch.randn((512,), generator=g).float(), torch.randn((128,), generator=g).float()
    y = F.relu(rnd(rnd(_f32conv(t2, w3[:, None, None, :]) + b3) + res))
    t1 = rnd(F.relu(_f32conv(y, w1[:, None, None, :]) + b1))
    (yv, ey), (tv, et) = cc.reference_pw_chain(t2, res, w3, b3, w1, b1, exact=False)
    assert ((y - yv).abs() <= ey).all() and ((t1 - tv).abs() <= et).all()


def _unpack_w2(w2, c, korder):
    """the packed [C, roundup(9 C, 64)] operand read in K order `korder` -> the logical [C, 3, 3, C] weight a kernel multiplies with"""
    w = w2[:, :9 * c]
    return w.reshape(c, c // 64, 3, 3, 64).permute(0, 2, 3, 1, 4).reshape(c, 3, 3, c) if korder else w.reshape(c, 3, 3, c)


def _simulated_c3_pair(x, w1, b12, w2, xo, shortcut, defect=None):
    """md_c3_pair as a correct kernel computes it from the header's operands -- fp32 convs, fp32 SiLU, T1 zero outside the image and
    rounded to bf16, the pre-shortcut value rounded to bf16, the shortcut added in fp32 and rounded again -> bf16 [N, H, W, C].
    defect: 'halo' T1's pixels outside the image are silu(b1) instead of 0; 'unrounded' the intermediate stays fp32; 'single' the
    shortcut is added before the rounding (one rounding instead of two); 'korder0' w2 is read in K order 0 whatever the width"""
    c = w1.shape[0]
    b1, b2 = b12[:c].float(), b12[c:].float()
    xs = x[..., xo:xo + c].float()
    t = F.silu(nhwc(F.conv2d(nchw(xs), w1[:, :c].float()[:, :, None, None])) + b1)
    t = t if defect == "unrounded" else t.to(BF).float()
    tp = F.pad(nchw(t), (1,) * 4)
    if defect == "halo":
        edge = torch.ones_like(tp[:, :1])
        edge[:, :, 1:-1, 1:-1] = 0
        tp = tp + edge * F.silu(b1).to(BF).float()[None, :, None, None]
    korder = 0 if c == 32 or defect == "korder0" else 1
    u = F.silu(nhwc(F.conv2d(tp, _unpack_w2(w2, c, korder).float().permute(0, 3, 1, 2))) + b2)
    if not shortcut:
        return u.to(BF)
    return (u + xs).to(BF) if defect == "single" else (u.to(BF).float() + xs).to(BF)


def _old_c3_tolerance_passes(got, x, w1l, b1, w2l, b2, xo, shortcut):
    """the judge of test_c3_pair_equals_two_launches_and_fp32: fp32 torch with bf16-rounded intermediates, |err| <= 2e-2 |y| + 3e-2"""
    c = w1l.shape[0]
    xs = x[..., xo:xo + c].float()
    t = F.silu(_f32conv(xs.double(), w1l[:, None, None, :]).float() + b1).to(BF).float()
    want = F.silu(_f32conv(t.double(), w2l, 1).float() + b2).to(BF).float()
    want = want + xs if shortcut else want
    return bool(((got.float() - want).abs() <= 2e-2 * want.abs() + 3e-2).all())


def test_c3_pair_contract_passes_a_correct_kernel_and_sees_four_defects():
    """On the draws the GPU test makes: the simulated kernel meets the exact regime's either-neighbour rule and the Gaussian bound at
    C = 32, 64 and 128; T1 not zeroed outside the image, an un-rounded intermediate, the shortcut added before the rounding and
    (C = 128) K order 0 instead of 1 each fail the exact regime.  The fp32 judge of test_c3_pair_equals_two_launches_and_fp32
    (|err| <= 2e-2 |y| + 3e-2), evaluated on the Gaussian draw, PASSES the un-rounded intermediate and the single rounding: it is
    several bf16 ulps wide at outputs of order 1, which is why the contract tests exist."""
    from tests.conv_checks import check, check_silu

    def exact_fails(case, defect):
        x, w1l, b1, w2l, b2 = _c3_draw(case, True)
        _, pre2, res = cc.reference_c3_pair(x, w1l, b1, w2l, b2, case[8], case[5], exact=True)
        w1, w2 = cc.c3_pair_weights(w1l, w2l)
        try:
            check_silu(_simulated_c3_pair(x, w1, torch.cat([b1, b2]), w2, case[8], case[5], defect), pre2, res)
        except AssertionError as e:
            return str(e)
        return None

    def gaussian(case, defect):
        """(inside the contract's bound, inside the old fp32 tolerance)"""
        x, w1l, b1, w2l, b2 = _c3_draw(case, False)
        w1, w2 = cc.c3_pair_weights(w1l, w2l)
        got = _simulated_c3_pair(x, w1, torch.cat([b1, b2]), w2, case[8], case[5], defect)
        y, bound = cc.reference_c3_pair(x, w1l, b1, w2l, b2, case[8], case[5], exact=False)
        return bool(((got.double() - y).abs() <= bound).all()), _old_c3_tolerance_passes(got, x, w1l, b1, w2l, b2, case[8], case[5])

    for name in ("c32_ragged", "c64_offsets", "c128_offsets_no_second_half", "c128_ragged", "c64_smaller_than_a_tile"):
        assert exact_fails(_c3_case(name), None) is None, name
        assert gaussian(_c3_case(name), None) == (True, True), name
    for name, defects in (("c32_ragged", ("halo", "unrounded", "single")), ("c128_offsets_no_second_half", ("halo", "unrounded", "single", "korder0"))):
        for defect in defects:
            why = exact_fails(_c3_case(name), defect)
            in_bound, old_passes = gaussian(_c3_case(name), defect)
            print(f"{name} {defect}: exact regime: {why}; Gaussian regime: {'inside' if in_bound else 'outside'} the bound; "
                  f"the fp32 tolerance {'passes' if old_passes else 'fails'} it")
            assert why is not None, (name, defect)
            if defect in ("unrounded", "single"):
                assert old_passes, (name, defect)


def _simulated_pw_chain(t2, res, w3, b3, w1, b1, defect=None):
    """md_pw_chain as a correct kernel computes it: fp32 GEMMs, y = relu(bf16(bf16(conv3 + b3) + res)), t1 = bf16(relu(conv1(y) + b1)).
    defect: 'fp32_y' conv1 reads the un-rounded fp32 y; 'relu_first' ReLU is applied before the residual add"""
    v = (t2.float() @ w3.float().t() + b3.float())
    if defect == "relu_first":
        y = (F.relu(v.to(BF).float()) + res.float()).to(BF)
    else:
        y = F.relu((v.to(BF).float() + res.float()).to(BF))
    y_in = F.relu(v + res.float()) if defect == "fp32_y" else y.float()
    return y, F.relu(y_in @ w1.float().t() + b1.float()).to(BF)


def test_pw_chain_contract_passes_a_correct_kernel_and_sees_two_defects():
    """the draw of test_pw_chain_gpu's exact regime (every second channel of b3 wide, so that y's roundings round) and a Gaussian one:
    the simulated kernel is bit-equal / within the bounds; conv1 on the un-rounded fp32 y and ReLU before the residual add each fail
    the exact regime"""
    from tests.conv_checks import Data, check

    d = Data(True, 7001, "cpu")
    t2, res = d.act((1, 5, 7, 128)), d.act((1, 5, 7, 512), hi=8)
    w3, w1, b3, b1 = d.weight((512, 128), 128), d.weight((128, 512), 512), d.bias(512, 512), d.bias(128, 128)
    b3[1::2] = torch.randint(-400, 401, (256,), generator=d.g).float()
    y_ref, t1_ref = cc.reference_pw_chain(t2, res, w3, b3, w1, b1)
    y, t1 = _simulated_pw_chain(t2, res, w3, b3, w1, b1)
    check(y, y_ref, True)
    check(t1, t1_ref, True)
    y, t1 = _simulated_pw_chain(t2, res, w3, b3, w1, b1, "fp32_y")
    check(y, y_ref, True)                                     # y itself is right: only t1 can show this defect
    with pytest.raises(AssertionError, match="outputs differ"):
        check(t1, t1_ref, True)
    y, t1 = _simulated_pw_chain(t2, res, w3, b3, w1, b1, "relu_first")
    with pytest.raises(AssertionError, match="outputs differ"):
        check(y, y_ref, True)
    d = Data(False, 7002, "cpu")
    t2, res = d.act((1, 5, 7, 128)), d.act((1, 5, 7, 512))
    w3, w1, b3, b1 = d.weight((512, 128), 128), d.weight((128, 512), 512), d.bias(512, 512), d.bias(128, 128)
    y, t1 = _simulated_pw_chain(t2, res, w3, b3, w1, b1)
    ref_y, ref_t1 = cc.reference_pw_chain(t2, res, w3, b3, w1, b1, exact=False)
    ry, rt = check(y, ref_y, False), check(t1, ref_t1, False)
    n, h, w, _ = t2.shape
    r1 = check(t1, cc.conv_stage(y.double(), 0.0, w1[:, None, None, :], b1, cc._plain(n, h, w, 512, 1, 1, 0, 128), 1), False)
    print(f"correct kernel, Gaussian regime: worst err / bound y {ry:.3f}, t1 {rt:.3f} (chain), {r1:.3f} (on its own y)")
