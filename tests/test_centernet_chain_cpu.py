"""No GPU: the judge of tests/centernet_checks.py judged.

Part A -- the restatement against PyTorch.  On configs/centernet/centernet_tiny_train.py's model the float64 restatement with every bf16
rounding switched off (judge(raw=True): the float64 fold as weights, the chain's exact value) against a plain torch.nn.functional float64
network (conv2d, batch_norm in eval form, zero pad + max_pool2d, conv_transpose2d) built from the same raw parameters; with dcn=True too,
the DCN layer written with F.grid_sample.  Two conditions, because a worst-case round-off bound carried through twenty layers' sum |w|
says nothing at the end: (1) every layer of the restatement equals the torch form of that layer on the same input within
2 (K + 8) 2^-53 sum |terms|, a derived bound; (2) end to end, per head slice, within 8 times the torch network's own float64 error (its
difference from a second evaluation with the BatchNorms folded): 3e-14 on hm, 1e-18 on wh and reg here -- and the same comparison rejects
a torch network with wh and reg swapped or a residual dropped.  The scatter transposed conv against F.conv_transpose2d at (k, s, p) = (4, 2, 1), (2, 2, 0), (4, 4, 0) on
1x1, 1x7, 5x1 and 5x7 inputs, cin 16, cout 24, within 2 K 2^-53 sum |x w|, K = (k / s)^2 cin; the float64 DCN definition against
sc.deform_cols on exact-regime draws (its masks 1 stand for float64 sigmoids within 2^-25 of 1: sc's docstring).

Part B -- planted faults.  The device is stood in for by an emulation of the C ABI (fake_call: md_conv2d from its attribute struct through
cc.conv_geometry with fp32 accumulation and the kernels' bf16 rounding points, md_maxpool2d, md_stem_pool, md_deform_cols as the bf16
rounding of sc.deform_cols), so graphs.py and nn_ops.py themselves run.  The clean models pass every check; each fault, a one-line mutation of
a copy of the model, of the emulated kernel or of the restatement, is reported by the check named here:
    wh and reg swapped in fuse_heads ............... `fused weights` (check_fused_weights) and `fused==unfused` (judge)
    a head2 block shifted by 64 columns ............ `fused weights` and `fused==unfused`
    two parity sub-kernels of a deconv exchanged ... `fold` (the kernel read back by the scatter pairing is not the folded one)
    pad_top 0 where 1 belongs ...................... `deconv readback` (a tap pairs rows the scatter definition does not)
    the residual of one BasicBlock dropped ......... `features==launches`
    BN eps 1e-5 where the module says 1e-3 ......... `fold`
    var where sqrt(var + eps) belongs .............. `fold`
    DCN offsets read as (x, y) ..................... `launch` (md_deform_cols) for the kernel; the restatement's own (x, y) reading leaves
                                                     sc.deform_cols"""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

from minddet_amd import _lib, graphs, nn_ops
from tests import centernet_checks as cn
from tests import conv_contract as cc
from tests import sample_contract as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulated library
# ---------------------------------------------------------------------------------------------------------------------------------
def _attrs(extra):
    return {f: getattr(extra, f) for f, _ in extra._fields_ if f != "tune"}


def fake_call(name, tensors, extra=None, stream=None, dcn_yx=True):
    if name == "md_conv2d":
        x, w, bias, res, out = tensors
        a = _attrs(extra)
        g = cc.conv_geometry([list(x.shape), list(w.shape), list(bias.shape), None if res is None else list(res.shape), list(out.shape)], a)
        rows = w.shape[0]
        wk = w[:, :g.kh * g.kw * g.cin].float()
        if a["korder"] == 1:
            wl = wk.reshape(rows, g.cin // 64, g.kh, g.kw, 64).permute(0, 2, 3, 1, 4).reshape(rows, g.kh, g.kw, g.cin)
        else:
            wl = wk.reshape(rows, g.kh, g.kw, g.cin)
        xs = x[..., g.x_c_off:g.x_c_off + g.cin].float().permute(0, 3, 1, 2)
        pb = (g.sub_h - 1) * g.stride + g.kh - g.pad_top - x.shape[1]
        pr = (g.sub_w - 1) * g.stride + g.kw - g.pad_left - x.shape[2]
        pre = F.conv2d(F.pad(xs, (g.pad_left, pr, g.pad_top, pb)), wl[:g.cout].permute(0, 3, 1, 2).contiguous(), bias[:g.cout].float(), g.stride)
        assert tuple(pre.shape[2:]) == (g.sub_h, g.sub_w)
        y = cc.epilogue(pre.permute(0, 2, 3, 1).double(), a["relu"], cc.residual_values(res, a, g))
        cc.out_view(out, g)[...] = y.to(BF)
    elif name == "md_maxpool2d":
        x, y = tensors
        assert extra.zero_pad
        y.copy_(F.max_pool2d(F.pad(x.float().permute(0, 3, 1, 2), (extra.pad,) * 4), extra.k, extra.stride).permute(0, 2, 3, 1))
    elif name == "md_stem_pool":
        x4, w, bias, y = tensors
        img = cc.stem_image(x4).float().permute(0, 3, 1, 2)
        wl = w.float().reshape(64, 7, 8, 4)[:, :, :7, :3].permute(0, 3, 1, 2).contiguous()
        t = F.relu(F.conv2d(img, wl, bias.float(), 2, 3)).to(BF).float()
        y.copy_(F.max_pool2d(t, 3, 2, 1).permute(0, 2, 3, 1))
    elif name == "md_deform_cols":
        x, off, cols = tensors
        T = extra.k * extra.k
        if not dcn_yx:                                     # the planted fault: the pair of tap t read as (dx, dy)
            off = off.clone()
            off[..., 0:2 * T:2], off[..., 1:2 * T:2] = off[..., 1:2 * T:2].clone(), off[..., 0:2 * T:2].clone()
        v, _, _ = sc.deform_cols(x, off, extra.k, extra.stride, extra.pad)
        cols.copy_(cc.bf16_rne(v).to(BF))
    else:
        raise AssertionError(f"no emulation of {name}")
    return 0


@pytest.fixture
def emulated(monkeypatch):
    monkeypatch.setattr(_lib, "call", fake_call)


def tiny(dcn):
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centernet", "centernet_tiny_train.py"))
    m = build_detector(dict(cfg.model, dcn=dcn), cfg.train_cfg, cfg.test_cfg).to("cpu")
    cn.pack_unfused(m, "cpu")
    return m


_MODELS = {}


def model(dcn=False):
    """a fresh copy of the packed tiny model (built once per variant)"""
    if dcn not in _MODELS:
        _MODELS[dcn] = tiny(dcn)
    return copy.deepcopy(_MODELS[dcn])


def images(h=32, w=64, stem_layout=False, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros((1, h, w, 8))
    x[..., :3] = torch.randn((1, h, w, 3), generator=g)
    x = x.to(BF)
    return nn_ops.to_stem_layout(x) if stem_layout else x


def reported(check, fn):
    with pytest.raises(cn.Fault) as ei:
        fn()
    assert ei.value.check == check, str(ei.value)


# ---------------------------------------------------------------------------------------------------------------------------------
# Part A
# ---------------------------------------------------------------------------------------------------------------------------------
EPS = 2.0 ** -53
_d = lambda t: torch.as_tensor(t).double()
nchw = lambda t: t.permute(0, 3, 1, 2)
nhwc = lambda t: t.permute(0, 2, 3, 1)


def _bn(t, p):
    return t if p is None else F.batch_norm(t, _d(p[2]), _d(p[3]), _d(p[0]), _d(p[1]), False, 0.0, p[4])


FOLDED = [False]     # the second evaluation of torch_net: the BatchNorm as a scale and shift folded into the conv's weights and bias


def _scale_shift(p, bias, cout):
    s = torch.ones(cout, dtype=torch.float64) if p is None else _d(p[0]) / torch.sqrt(_d(p[3]) + p[4])
    b = torch.zeros(cout, dtype=torch.float64) if p is None else _d(p[1]) - _d(p[2]) * s
    return s, b if bias is None else b + _d(bias) * s


def torch_conv(c, t):
    """Conv2d (+ bias) + eval BatchNorm of a ConvModule from its raw parameters, NCHW float64"""
    if FOLDED[0]:
        s, b = _scale_shift(c.bn, c.bias, c.cout)
        return F.conv2d(t, _d(c.weight) * s.view(-1, 1, 1, 1), b, c.stride, c.pad)
    return _bn(F.conv2d(t, _d(c.weight), None if c.bias is None else _d(c.bias), c.stride, c.pad), c.bn)


def torch_deconv(c, t):
    if FOLDED[0]:
        s, b = _scale_shift(c.bn, None, c.cout)
        return F.conv_transpose2d(t, _d(c.weight_t) * s.view(1, -1, 1, 1), b, c.stride, c.pad)
    return _bn(F.conv_transpose2d(t, _d(c.weight_t), None, c.stride, c.pad), c.bn)


def torch_dcn(c, t):
    """DCNv2 + eval BatchNorm in plain torch: the offset conv, per tap F.grid_sample (bilinear, zeros, align_corners=True: the sampling rule
    sample_contract states) at base + (dy, dx) times the sigmoid of the tap's logit, then the k x k weights as one einsum"""
    off = F.conv2d(t, _d(c.offset_weight), _d(c.offset_bias), c.stride, c.pad)
    (N, C, H, W), k, T = t.shape, c.k, c.k * c.k
    ys = (torch.arange(off.shape[2]) * c.stride - c.pad).double()[:, None]
    xs = (torch.arange(off.shape[3]) * c.stride - c.pad).double()[None, :]
    cols = []
    for tap in range(T):
        y, x = ys + tap // k + off[:, 2 * tap], xs + tap % k + off[:, 2 * tap + 1]
        grid = torch.stack([2 * x / (W - 1) - 1, 2 * y / (H - 1) - 1], -1)
        cols.append(F.grid_sample(t, grid, mode="bilinear", padding_mode="zeros", align_corners=True) * torch.sigmoid(off[:, 2 * T + tap])[:, None])
    if FOLDED[0]:
        s, b = _scale_shift(c.bn, None, c.cout)
        return torch.einsum("nctyx,oct->noyx", torch.stack(cols, 2), (_d(c.weight) * s.view(-1, 1, 1, 1)).reshape(c.cout, C, T)) + b.view(1, -1, 1, 1)
    return _bn(torch.einsum("nctyx,oct->noyx", torch.stack(cols, 2), _d(c.weight).reshape(c.cout, C, T)), c.bn)


def torch_net(m, x, order=cn.HEADS, no_residual=None):
    """the reference's network in plain float64 torch.nn.functional from the raw parameters; x [N, 3, H, W] -> [N, nc + 4, H/4, W/4].
    order / no_residual: the two faults planted in THIS network (head order; the (stage, block) whose residual is dropped)"""
    bb = m.backbone
    t = F.max_pool2d(F.pad(F.relu(torch_conv(bb.conv1, x)), (1, 1, 1, 1)), 3, 2)
    for si, st in enumerate(bb.stages):
        for bi, b in enumerate(st):
            r = t if b.downsample is None else torch_conv(b.downsample, t)
            u = torch_conv(b.conv2, F.relu(torch_conv(b.conv1, t)))
            t = F.relu(u if (si, bi) == no_residual else u + r)
    for c in m.neck:
        t = F.relu(torch_deconv(c, t) if hasattr(c, "weight_t") else torch_dcn(c, t) if hasattr(c, "offset_weight") else torch_conv(c, t))
    return torch.cat([torch_conv(m.heads[n][1], F.relu(torch_conv(m.heads[n][0], t))) for n in order], 1)


def _terms(c, x, weight=None, bias="bias"):
    """sum |x| |w'| + |beta| + |mean scale| + |bias scale| of one layer, NCHW: the magnitudes every rounding of either evaluation acts on
    (the restatement folds, torch normalises after the conv: |conv| <= sum |x| |w|, so the unfolded terms are no larger)"""
    w = _d(c.weight if weight is None else weight)
    b = getattr(c, bias, None)
    s = torch.ones(w.shape[0], dtype=torch.float64)
    mag = torch.zeros(w.shape[0], dtype=torch.float64)
    if c.bn is not None and weight is None:
        s = _d(c.bn[0]).abs() / torch.sqrt(_d(c.bn[3]) + c.bn[4])
        mag = _d(c.bn[1]).abs() + (_d(c.bn[2]) * s).abs()
    if b is not None:
        mag = mag + (_d(b) * s).abs()
    return w.abs() * s.view(-1, 1, 1, 1), mag.view(1, -1, 1, 1)


@pytest.mark.parametrize("dcn", [False, True], ids=["plain", "dcn"])
def test_every_layer_of_the_restatement_equals_torch_on_the_same_input(dcn):
    """Layer by layer: each layer of judge(raw=True) against the torch.nn.functional form of that layer from the raw parameters on the SAME
    input, within 2 (K + 8) 2^-53 (sum |x| |w'| + |beta| + |mean scale| + |bias scale| + |residual|): K + 1 additions per output on either
    side in any order (gamma_K each, Higham eq. 3.5), the fold's or the BatchNorm's at most six roundings, the residual add; both sides err.
    The pool is exact.  A DCN layer adds what the two sides' offsets may differ by: e_off = the same bound for the offset conv; the
    coordinate passes through grid_sample's normalisation, 2 c / (W - 1) - 1 and back, at most eight roundings of values below |c| + W;
    a sample moves by at most (L_y + L_x) e_c (L: largest adjacent difference of the zero-extended channel), a mask by e_off / 4; carried
    through sum |w'|."""
    m = model(dcn)
    x = images(64, 96)
    trace = cn.judge(m, x, launch=False, raw=True)["trace"]
    assert [k for k, *_ in trace].count("conv") == 20 + 6 + (0 if dcn else 3) and [k for k, *_ in trace].count("deconv") == 3
    assert [k for k, *_ in trace].count("dcn") == (3 if dcn else 0) and trace[1][0] == "pool"
    for kind, c, t, res, relu, y in trace:
        xin = nchw(t)
        if kind == "pool":
            assert torch.equal(nchw(y), F.max_pool2d(F.pad(xin, (1, 1, 1, 1)), 3, 2))
            continue
        if kind == "conv":
            xin = xin[:, :c.cin]
            z = torch_conv(c, xin)
            aw, mag = _terms(c, xin)
            absum, K = F.conv2d(xin.abs(), aw, None, c.stride, c.pad) + mag, c.k * c.k * c.cin
        elif kind == "deconv":
            z = torch_deconv(c, xin)
            aw, mag = _terms(c, xin, c.weight_t.permute(1, 0, 2, 3), bias="none")
            if c.bn is not None:
                sc_ = _d(c.bn[0]).abs() / torch.sqrt(_d(c.bn[3]) + c.bn[4])
                aw, mag = aw * sc_.view(-1, 1, 1, 1), (_d(c.bn[1]).abs() + (_d(c.bn[2]) * sc_).abs()).view(1, -1, 1, 1)
            absum, K = F.conv_transpose2d(xin.abs(), aw.permute(1, 0, 2, 3), None, c.stride, c.pad) + mag, 4 * c.cin
        else:
            z = torch_dcn(c, xin)
            aw, mag = _terms(c, xin)
            K = 9 * c.cin
            xmax = xin.abs().amax((2, 3))                                                   # [N, C]: a sample is a convex combination
            absum = (aw.sum((2, 3))[None] * xmax[:, None, :]).sum(2)[:, :, None, None] + mag
            wo, bo = _d(c.offset_weight).abs(), _d(c.offset_bias).abs().view(1, -1, 1, 1)
            e_off = float((2 * (K + 8) * EPS * (F.conv2d(xin.abs(), wo, None, c.stride, c.pad) + bo)).max())
            off = F.conv2d(xin, _d(c.offset_weight), _d(c.offset_bias), c.stride, c.pad)
            e_c = e_off + 8 * EPS * (float(off[:, :18].abs().max()) + 2 * max(xin.shape[2:]) + 2)
            Ly, Lx = cn._adjacent(t)
            moved = (Ly + Lx) * e_c + xmax * e_off / 4                                      # [N, C]
            absum = absum + (aw.sum((2, 3))[None] * moved[:, None, :]).sum(2)[:, :, None, None] / (2 * (K + 8) * EPS)
        if res is not None:
            z, absum = z + nchw(res), absum + nchw(res).abs()
        z = F.relu(z) if relu else z
        err = (nchw(y)[:, :z.shape[1]] - z).abs()
        assert bool((err <= 2 * (K + 8) * EPS * absum).all()), (kind, float((err / absum).max() / EPS))
        assert float(err.max()) <= 1e-9 * float(z.abs().max()), kind                        # (the bound is round-off, not a tolerance)


@pytest.mark.parametrize("dcn", [False, True], ids=["plain", "dcn"])
def test_restatement_equals_a_plain_torch_network(dcn):
    """End to end, which holds the restatement's own graph walk, residuals and channel order.  Worst-case round-off bounds grow by sum |w|
    per layer and say nothing after twenty layers, so the tolerance is the reference's own float64 error instead: the same torch network
    evaluated a second time with every BatchNorm folded into its conv as a scale and shift (mathematically equal, rounded differently in
    every layer).  Per head slice, the restatement differs from the torch network by at most 8 times the largest difference of the two
    torch evaluations in that slice (the maximum over 768 to 1920 outputs of one round-off sample against that of another; the 8 is
    margin for the two maxima, and the planted faults below miss it by ten orders).  Then the two faults planted in the torch network,
    which the comparison must see."""
    m = model(dcn)
    x = images(64, 96)
    xin = nchw(x[..., :3].double()).contiguous()
    out = cn.judge(m, x, launch=False, raw=True)
    want = nhwc(torch_net(m, xin))
    assert out["value"].shape == want.shape == (1, 16, 24, 9)
    FOLDED[0] = True
    try:
        again = nhwc(torch_net(m, xin))
    finally:
        FOLDED[0] = False
    slices = {"hm": slice(0, 5), "wh": slice(5, 7), "reg": slice(7, 9)}

    def agrees(value):
        return all(float((value[..., sl] - want[..., sl]).abs().max()) <= 8 * float((again[..., sl] - want[..., sl]).abs().max()) for sl in slices.values())

    ref_err = {n: float((again[..., sl] - want[..., sl]).abs().max()) for n, sl in slices.items()}
    assert all(0 < v < 1e-12 for v in ref_err.values()), ref_err                             # round-off: there, and nothing more
    assert 0 < float(want[..., 5:].abs().max()) < 0.05                                        # wh, reg: of order 1e-3 at the default initialisation
    assert agrees(out["value"]), {n: float((out["value"][..., sl] - want[..., sl]).abs().max()) for n, sl in slices.items()}
    assert not agrees(nhwc(torch_net(m, xin, order=("hm", "reg", "wh"))))                    # planted in torch_net: wh and reg swapped
    assert not agrees(nhwc(torch_net(m, xin, no_residual=(3, 1))))                           # planted in torch_net: a residual dropped


@pytest.mark.parametrize("ksp", [(4, 2, 1), (2, 2, 0), (4, 4, 0)], ids=lambda v: "k%d_s%d_p%d" % v)
@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (5, 1), (5, 7)], ids=lambda v: "%dx%d" % v)
def test_scatter_transposed_conv_equals_torch(ksp, hw):
    k, s, p = ksp
    g = torch.Generator().manual_seed(k * 100 + s * 10 + hw[0] + hw[1])
    x = torch.randn((2,) + hw + (16,), generator=g, dtype=torch.float64)
    w = torch.randn((16, 24, k, k), generator=g, dtype=torch.float64)
    got = cn.deconv_scatter(x, w, s, p)
    want = F.conv_transpose2d(x.permute(0, 3, 1, 2), w, None, s, p).permute(0, 2, 3, 1)
    assert got.shape == want.shape == (2, (hw[0] - 1) * s - 2 * p + k, (hw[1] - 1) * s - 2 * p + k, 24)
    absum = cn.deconv_scatter(x.abs(), w.abs(), s, p)
    assert bool(((got - want).abs() <= 2 * (k // s) ** 2 * 16 * 2.0 ** -53 * absum).all())
    # the exact regime of deconv_stage: small integers stay exact, and the epilogue rounds nothing away
    xi = torch.randint(-2, 3, x.shape, generator=g).double()
    wi = torch.randint(-1, 2, w.shape, generator=g).double()
    y, none = cn.deconv_stage(xi, None, wi, torch.zeros(24), s, p, 1)
    assert none is None and torch.equal(y, F.relu(F.conv_transpose2d(xi.permute(0, 3, 1, 2), wi, None, s, p)).permute(0, 2, 3, 1))


@pytest.mark.parametrize("ksp", [(3, 1, 1), (3, 2, 1)], ids=lambda v: "k%d_s%d_p%d" % v)
def test_dcn_definition_equals_sample_contract(ksp):
    k, s, p = ksp
    x, off, _ = sc.gen_dcn((2, 5, 7), 8, k, s, p, False, True, 11, "cpu")
    acc, m, _ = cn.dcn_exact(x.double(), off.double(), k, s, p)
    v, e, _ = sc.deform_cols(x, off, k, s, p)
    assert bool((e[~torch.isnan(v)] == 0).all())
    ok = ~torch.isnan(v)
    tol = 2.0 ** -25 * (acc.abs() * m[..., None]).reshape(v.shape) + 2.0 ** -50 * acc.abs().reshape(v.shape)
    assert bool((((acc * m[..., None]).reshape(v.shape) - v).abs()[ok] <= tol[ok]).all())
    acc, m, _ = cn.dcn_exact(x.double(), off.double(), k, s, p, yx=False)                    # the restatement's own (x, y) reading
    assert not bool((((acc * m[..., None]).reshape(v.shape) - v).abs()[ok] <= tol[ok]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# Part B
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dcn", [False, True], ids=["plain", "dcn"])
def test_clean_model_passes_every_check(emulated, dcn):
    m = model(dcn)
    out = cn.check_all(m, images())
    assert out["chain"] <= 1 and all(v <= 1 for v in out["launches"].values())
    assert {"conv 7x7 s2", "maxpool 3x3 s2", "conv 3x3 s2", "conv 1x1 s2 downsample", "conv 3x3 s1 + residual", "deconv k4 s2 p1", "head 3x3",
            "head 1x1", "head1 (fused 3x3)", "head2 (fused 1x1)"} <= set(out["launches"])
    assert ({"dcn offset conv", "md_deform_cols", "dcn GEMM K=9C"} <= set(out["launches"])) == dcn
    cn.report(f"emulated tiny dcn={dcn}", out)


def test_clean_model_passes_in_the_stem_layout(emulated):
    out = cn.check_all(model(), images(32, 64, stem_layout=True))
    assert "md_stem_pool" in out["launches"] and "conv 7x7 s2" not in out["launches"]


@pytest.mark.parametrize("ksp", [(4, 2, 1), (2, 2, 0), (4, 4, 0)], ids=lambda v: "k%d_s%d_p%d" % v)
def test_conv_transpose_check_passes_the_emulation_and_sees_a_wrong_parity(emulated, ksp):
    """cn.check_conv_transpose (the GPU test's condition on nn_ops.conv_transpose2d alone) in both regimes on the emulated library, and a
    launch that writes the wrong output parity"""
    from tests.conv_checks import Data

    k, s, p = ksp
    for exact in (True, False):
        d = Data(exact, 70 + k + int(exact), "cpu")
        x = d.act((2, 5, 7, 16))
        init = graphs.ParamInit(k)
        wt, bn = (d.weight((16, 24, k, k), k).float(), None) if exact else (init.conv(16, 24, k, 0.1), init.bn(24, 1e-3))
        pct = nn_ops.pack_conv_transpose(wt, bn=bn, stride=s, pad=p, relu=True)
        assert cn.check_conv_transpose(pct, wt, bn, p, x, exact) <= 1
        pct.subs[0][1]["px"], pct.subs[1][1]["px"] = pct.subs[1][1]["px"], pct.subs[0][1]["px"]
        with pytest.raises(AssertionError):
            cn.check_conv_transpose(pct, wt, bn, p, x, exact)


def _refuse(m, order=cn.HEADS, shift=None):
    """CenterNet.fuse_heads with one line changed: the order of the 64-channel bands, or the column band of one head2 block"""
    hc = m.head_conv
    m.head1.weight = torch.cat([m.heads[n][0].weight for n in order], 0)
    m.head1.bias = torch.cat([m.heads[n][0].bias for n in order], 0)
    w2, b2, o = torch.zeros((m.n_out, 3 * hc, 1, 1)), torch.zeros((m.n_out,)), 0
    for i, n in enumerate(order):
        c2 = m.heads[n][1]
        col = (i + 1 if n == shift else i) * hc
        w2[o:o + c2.cout, col:col + hc] = c2.weight
        b2[o:o + c2.cout] = c2.bias
        o += c2.cout
    m.head2.weight, m.head2.bias = w2, b2
    for c in (m.head1, m.head2):
        c.to("cpu")


def test_swapped_and_shifted_head_blocks_are_reported(emulated):
    m = model()
    _refuse(m)
    cn.check_fused_weights(m)                                                                # the helper itself fuses correctly
    for kw in (dict(order=("hm", "reg", "wh")), dict(shift="wh")):
        m = model()
        _refuse(m, **kw)
        cn.check_folding(m)                                                                  # head1 / head2 hold what they were given
        reported("fused weights", lambda: cn.check_fused_weights(m))
        reported("fused==unfused", lambda: cn.judge(m, images()))


def test_exchanged_parities_and_a_wrong_pad_top_are_reported(emulated):
    m = model()
    d = m.neck[1]
    assert [(s["py"], s["px"], s["pad_top"], s["pad_left"]) for _, s in d.packed.subs] == [(0, 0, 1, 1), (0, 1, 1, 0), (1, 0, 0, 1), (1, 1, 0, 0)]
    cn.check_module_fold(d, "neck.1")
    subs = d.packed.subs
    d.packed.subs = [(subs[3][0], subs[0][1]), subs[1], subs[2], (subs[0][0], subs[3][1])]
    reported("fold", lambda: cn.check_module_fold(d, "neck.1"))
    d.packed.subs = [(subs[0][0], dict(subs[0][1], pad_top=0))] + subs[1:]
    reported("deconv readback", lambda: cn.check_module_fold(d, "neck.1"))
    reported("deconv readback", lambda: cn.judge(m, images()))


class _NoResidual(graphs.BasicBlock):
    def __call__(self, x):
        return self.conv2(self.conv1(x))


def test_a_weight_on_a_padding_input_channel_of_a_deconv_is_reported():
    init = graphs.ParamInit(3)
    wt, bn = init.conv(12, 16, 4, 0.1), init.bn(16, 1e-3)                                    # cin 12: packed as 16 input channels
    pct = nn_ops.pack_conv_transpose(wt, bn=bn, stride=2, pad=1, relu=True)
    d = cn._Deconv(pct, wt, bn, 1)
    assert pct.subs[0][0].cin == 16
    cn.check_module_fold(d)
    pct.subs[2][0].w[3, 13] = 0.5
    reported("fold", lambda: cn.check_module_fold(d))


def test_a_dropped_residual_is_reported(emulated):
    m = model()
    m.backbone.stages[3][1].__class__ = _NoResidual
    cn.check_folding(m)
    reported("features==launches", lambda: cn.judge(m, images()))


def test_a_wrong_eps_and_a_wrong_denominator_are_reported(monkeypatch):
    m = model()
    c = m.backbone.stages[1][0].conv1
    c.bn = c.bn[:4] + (1e-3,)                                                                # the module says 1e-3 ...
    c.to("cpu")
    cn.check_module_fold(c)
    c.packed = nn_ops.pack_conv(c.weight, bias=c.bias, bn=c.bn[:4] + (1e-5,), stride=c.stride, pad=c.pad, relu=c.act)   # ... the pack 1e-5
    reported("fold", lambda: cn.check_module_fold(c))
    # the models' own eps is 1e-5: against half a bf16 ulp a weight sees it only next to a tie, but the bias has no bf16 term and sees any
    # relative change of the scale above gamma_6 (|beta| + |mean scale|) / |mean scale| (3.6e-7 with beta = 0); eps 0 moves it by 3e-6 to 1e-5
    c = m.backbone.stages[0][0].conv1
    cn.check_module_fold(c)
    c.packed = nn_ops.pack_conv(c.weight, bias=c.bias, bn=c.bn[:4] + (0.0,), stride=c.stride, pad=c.pad, relu=c.act)
    reported("fold", lambda: cn.check_module_fold(c))
    _, b64, _, eb = cn.fold64(c.weight, c.bias, c.bn)
    assert bool(((c.packed.bias[:c.cout].double() - b64).abs() > eb).all())                  # every channel's bias alone is outside its bound

    def fold_by_var(weight, bias, bn):
        gamma, beta, mean, var, eps = bn
        scale = gamma / (var + eps)                                                          # var where sqrt(var + eps) belongs
        return weight * scale.view(-1, 1, 1, 1), beta - mean * scale

    for mod in (m.backbone.stages[2][1].conv2, m.neck[3], m.backbone.conv1):
        cn.check_module_fold(mod)
        with monkeypatch.context() as mp:
            mp.setattr(nn_ops, "_fold_bn", fold_by_var)
            mod.to("cpu")
        reported("fold", lambda: cn.check_module_fold(mod))
    m = model()
    with monkeypatch.context() as mp:
        mp.setattr(nn_ops, "_fold_bn", fold_by_var)
        m.backbone.to("cpu")
    reported("fold", lambda: cn.check_module_fold(m.backbone.conv1, "conv1", m.backbone.stem))


def test_dcn_offsets_read_as_xy_are_reported(monkeypatch):
    m = model(dcn=True)
    monkeypatch.setattr(_lib, "call", lambda *a, **k: fake_call(*a, **k, dcn_yx=False))
    with pytest.raises(cn.Fault) as ei:
        cn.judge(m, images())
    assert ei.value.check == "launch" and "md_deform_cols" in str(ei.value)
