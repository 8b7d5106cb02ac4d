"""Shared by tests/test_centernet_chain_cpu.py and tests/test_centernet_chain_gpu.py: graphs.CenterNet.features restated in float64 from the
reference's model definition (centernet/src/resnet.py:109-252, centernet_det.py:29-174) and the module's RAW parameters, in the style of
tests/neck_checks.py.  Works on CPU and GPU tensors alike; every tolerance comes from tests/conv_contract.py (cc) or tests/sample_contract.py
(sc).  Each condition raises Fault, whose `check` names the condition that failed.

The path: conv7x7/s2/p3 + BN + ReLU, zero pad 1 + MaxPool 3x3/s2; four stages of two BasicBlocks (conv-BN-ReLU, conv-BN, + x or + conv1x1/s2-BN
of x, ReLU); three times (3x3 DCNv2 or plain conv + BN + ReLU, Conv2dTranspose 4x4/s2/p1 + BN + ReLU); the three UNFUSED heads of model.heads
(3x3 + bias + ReLU, 1x1 + bias); channels hm[0:nc] | wh | reg.

fold (check_folding).  The fold of (weight, gamma, beta, mean, var, eps) is computed here in float64 and compared with the logical weights
and bias the device holds, read back from the packed tensors (unpack: the inverse of cc.pack_weight, asserted to round-trip; the stem's
one-launch form through cc.pack_stem_pool's layout; a transposed conv through its sub-pixel packs, see deconv_logical).  nn_ops._fold_bn is
not used.  Bound, with u = 2^-24 and gamma_n = n u / (1 - n u) (Higham eq. 3.1: n roundings of relative size u): the package's fold
computes, in fp32, t = var + eps (one add, u; eps itself is rounded to fp32, at most u eps / (var + eps) <= u more), r = sqrt(t) (the
square root halves the 2 u that t carries and rounds once: 2 u), scale = gamma / r (one divide: 3 u), w' = w scale (one multiply: 4 u):
|w'_fp32 - w'_64| <= gamma_4 |w'_64|, and the device holds the bf16 nearest w'_fp32:
    |w_dev - w'_64| <= gamma_4 |w'_64| + bf16_quantum(|w'_64| (1 + gamma_4)) / 2.
Bias: b' = beta - mean scale (+ bias scale): each term sees the 3 u of scale, its product, and one subtraction (and one addition more with a
conv bias): |b_dev - b'_64| <= gamma_6 (|beta| + |mean scale| + |bias scale|), no bf16 term.  Without a BatchNorm the weight is the bf16
nearest the fp32 weight (half a bf16 ulp) and the bias is exact.  Padding channels and rows are exact zeros.  Sensitivity: a weight sees a
relative change of its scale below 2^-9 only next to a bf16 tie; the bias, with no bf16 term, sees any above gamma_6 (|beta| + |mean scale|)
/ |mean scale| (3.6e-7 with beta = 0, mean != 0), so an eps of 0 for 1e-5 (3e-6 to 1e-5 of the scale at var in [0.5, 1.5]) is seen there.  After this check the launches and
the chain use the device's bf16 weights, as neck_checks.logical does.

launch by launch (judge).  The judge walks the reference's graph itself and runs every module ALONE on the device's own input of that module;
its output is held to cc.conv_stage (convs, the residual convs with the device's residual), cc.reference_stem_pool (the one-launch stem), bit
for bit cc.max_pool (the pool), sc.deform_cols + sc.check (md_deform_cols on the device's offsets) and the scatter definition of the
transposed conv (deconv_stage: y[n, iy s - p + ky, ix s - p + kx, co] += x[n, iy, ix, ci] w[ci, co, ky, kx], never the parity decomposition;
the bound is cc.gaussian_bound with the (k / s)^2 cin + 1 terms of one output).  err / bound <= 1, the worst kept per kind of launch.  The
real plumbing (graphs.ResNet / BasicBlock / CenterNet.features) is then held to the judge's: model.features(images) equals the tensor rebuilt
from the single launches bit for bit (`features==launches`).

the chain.  The exact float64 value of the whole path and cc's accumulated bound (fp32 accumulation, one bf16 rounding per layer, carried
through the following layers' |w|; through the max pool as the max of the bounds).  Through a DCN layer (dcn_chain): the device samples its
own x' (|x' - x| <= e_x) at its own coordinates c' (|c' - c| <= e_c: the offset conv's bound plus the fp32 roundings of the coordinate).
Bilinear interpolation B of the zero-extended image is continuous and piecewise linear with slopes at most the largest difference L of
adjacent pixels (sc's module docstring), and a convex combination: |B_x'(c') - B_x(c)| <= max e_x + min(L_y e_cy + L_x e_cx, 2 max |x|), plus
sc.SAMPLE max(|x| + e_x) + sc.TINY for the kernel's sampling arithmetic; the mask sigmoid has slope <= 1/4 and sc.mask_value's fp32 term; the
column product and its bf16 rounding as in sc.bound.  No number of its own.  The chain's VALUE is what tests/test_centernet_chain_cpu.py holds
to a plain torch network (layer by layer within float64 round-off, end to end within the torch network's own float64 error; DCN included);
its BOUND is asserted on the device and, as said next, pins nothing.

Which condition pins what: through some twenty randomly initialised layers the chain bound grows by the layers' sum |w| each time and ends
above the head values (the printed chain ratio is far below 1 for that reason), so it cannot separate `wh` from `reg` (both of order 1e-3
at the default initialisation).  They are pinned by the launch-by-launch condition on head1 and head2 (each 3x3 and 1x1 head launch on
the device's own input, within one conv's bound, a fraction of a bf16 ulp of the value) together with `fused==unfused` (each channel slice of
head2(head1(x)) equals the unfused head's two launches) and `fused weights`.  Measured on an MI355X over the cases of
tests/test_centernet_chain_gpu.py (its docstring has the table): chain 1.2e-36 to 4.0e-33; head 3x3 0.939 to 0.981, head 1x1 0.993 to 0.998,
head1 0.939 to 0.981, head2 0.983 to 0.993 (a ratio near 1 is one output next to a bf16 tie), fused == unfused bit for bit."""
import torch

from tests import conv_contract as cc
from tests import sample_contract as sc

U = 2.0 ** -24
HEADS = ("hm", "wh", "reg")


def gamma(n):
    return n * U / (1.0 - n * U)


class Fault(AssertionError):
    def __init__(self, check, detail=""):
        super().__init__(f"{check}: {detail}")
        self.check = check


def _bits(t):
    return t.contiguous().view(torch.int16)


def _as_bits(v):
    """float64 values that are bf16 numbers -> their bit patterns"""
    return v.to(torch.bfloat16).contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------------------------
# the fold in float64 and the device's logical weights
# ---------------------------------------------------------------------------------------------------------------------------------
def fold64(weight, bias, bn):
    """weight [cout, ...] raw, bias [cout] or None, bn = (gamma, beta, mean, var, eps) or None -> (w', b', bound on the fp32 fold of w',
    bound on that of b'), float64 (see the module docstring)"""
    w = weight.detach().double()
    cout = w.shape[0]
    if bn is None:
        b = torch.zeros(cout, dtype=torch.float64) if bias is None else bias.detach().double()
        return w, b, torch.zeros_like(w), torch.zeros_like(b)
    g, beta, mean, var, eps = bn
    s = torch.as_tensor(g).double() / torch.sqrt(torch.as_tensor(var).double() + float(eps))
    ms = torch.as_tensor(mean).double() * s
    b = torch.as_tensor(beta).double() - ms
    mag = torch.as_tensor(beta).double().abs() + ms.abs()
    if bias is not None:
        b = b + bias.detach().double() * s
        mag = mag + (bias.detach().double() * s).abs()
    w = w * s.view(-1, *([1] * (w.dim() - 1)))
    return w, b, gamma(4) * w.abs(), gamma(6) * mag


def unpack(pc):
    """nn_ops.PackedConv -> (logical weight [cout_o, kh, kw, cin_p] float64 of the bf16 values, fp32 bias [cout_o]): the inverse of
    cc.pack_weight, asserted to round-trip (so the K padding and the rows past cout_o are exact zeros)"""
    rows, kpad = pc.w.shape
    kh, kw, cin, korder = pc.kh, pc.kw, pc.cin, getattr(pc, "korder", 0)
    w = pc.w[:, :kh * kw * cin].double()
    wl = w.reshape(rows, cin // 64, kh, kw, 64).permute(0, 2, 3, 1, 4).reshape(rows, kh, kw, cin) if korder == 1 else w.reshape(rows, kh, kw, cin)
    if not torch.equal(cc.pack_weight(wl, korder, kpad, rows), pc.w.double()) or bool(wl[pc.cout:].any()) or bool(pc.bias[pc.cout:].any()):
        raise Fault("fold", "the pack does not round-trip through cc.pack_weight, or its padding is not zero")
    return wl[:pc.cout], pc.bias[:pc.cout]


def stem_logical(ps):
    """nn_ops.PackedStem -> ([64, 7, 7, 3] float64, bias): cc.pack_stem_pool's layout read back"""
    wp = ps.w.double().reshape(64, 7, 8, 4)
    wl = wp[:, :, :7, :3]
    if not torch.equal(cc.pack_stem_pool(wl), ps.w.double()):
        raise Fault("fold", "the stem pack has weights outside cc.pack_stem_pool's layout")
    return wl.contiguous(), ps.bias


def deconv_logical(pct, pad):
    """nn_ops.PackedConvT -> (w [cin, cout_o, k, k] float64, bias): the full transposed-conv kernel the sub-pixel launches amount to by
    the SCATTER definition.  The launch of parity (py, px) with pad_top pt writes output row oy = s ho + py from input rows iy = ho - pt + i
    (tap i); the scatter definition pairs oy and iy through kernel row ky = oy - s iy + pad = py + pad + s (pt - i).  A tap that names a
    row outside [0, k), or a kernel entry named twice or never, is a fault; every sub-pixel pack carries the same bias."""
    k, s = pct.k, pct.stride
    cout = pct.subs[0][0].cout
    dev = pct.subs[0][0].w.device
    w = torch.zeros((pct.cin, cout, k, k), dtype=torch.float64, device=dev)
    seen = torch.zeros((k, k), dtype=torch.int64)
    bias = None
    for pc, m in pct.subs:
        wl, b = unpack(pc)                                                        # [cout, nty, ntx, cin]
        if bool(wl[..., pct.cin:].any()):
            raise Fault("fold", "a sub-pixel pack has a non-zero weight on a padding input channel")
        if bias is not None and not torch.equal(b, bias):
            raise Fault("deconv readback", "the sub-pixel launches carry different biases")
        bias = b
        for i in range(pc.kh):
            for j in range(pc.kw):
                ky, kx = m["py"] + pad + s * (m["pad_top"] - i), m["px"] + pad + s * (m["pad_left"] - j)
                if not (0 <= ky < k and 0 <= kx < k):
                    raise Fault("deconv readback", f"parity ({m['py']}, {m['px']}) tap ({i}, {j}) pairs rows the scatter definition does not")
                seen[ky, kx] += 1
                w[:, :, ky, kx] = wl[:, i, j, :pct.cin].t()
    if not bool((seen == 1).all()):
        raise Fault("deconv readback", f"kernel entries covered {seen.tolist()} times")
    return w, bias


def _held(check, what, dev, want, bound):
    err = (dev.double().cpu() - want).abs()
    if not bool((err <= bound).all()):
        i = tuple(int(v) for v in (err > bound).nonzero()[0])
        raise Fault(check, f"{what}: {int((err > bound).sum())} of {err.numel()} entries past the bound; first at {i}: device {float(dev.double().cpu()[i])!r}, "
                           f"float64 fold {float(want[i])!r} +- {float(bound[i]):.3e}")


def _weight_bound(w64, ew, has_bn):
    return ew + cc.bf16_quantum(w64.abs() * (1.0 + (gamma(4) if has_bn else 0.0))) / 2


def check_module_fold(m, name="", stem=None):
    """one ConvModule / DeformConvModule / DeconvModule: the device's logical weights and bias within the fold's bound of the float64 fold;
    padding exactly zero.  stem: the backbone's nn_ops.PackedStem of this module, judged as well."""
    if hasattr(m, "weight_t"):
        w64, b64, ew, eb = fold64(m.weight_t.permute(1, 0, 2, 3), None, m.bn)                 # [cout, cin, k, k]
        wd, bd = deconv_logical(m.packed, m.pad)
        packs = [(wd.permute(1, 2, 3, 0), bd, w64.permute(0, 2, 3, 1), b64, ew.permute(0, 2, 3, 1), eb, m.bn)]
    else:
        w64, b64, ew, eb = fold64(m.weight, m.bias, m.bn)
        packs = [unpack(m.packed) + (w64.permute(0, 2, 3, 1), b64, ew.permute(0, 2, 3, 1), eb, m.bn)]
        if stem is not None:
            packs.append(stem_logical(stem) + packs[0][2:])
        if hasattr(m, "offset_weight"):
            wo, bo, ewo, ebo = fold64(m.offset_weight, m.offset_bias, None)
            packs.append(unpack(m.packed_offset) + (wo.permute(0, 2, 3, 1), bo, ewo.permute(0, 2, 3, 1), ebo, None))
    for wd, bd, w, b, e_w, e_b, bn in packs:
        co, kh, kw, ci = w.shape
        wd, bd = wd.cpu(), bd.double().cpu()
        if tuple(wd.shape[1:3]) != (kh, kw) or wd.shape[0] < co or wd.shape[3] < ci:
            raise Fault("fold", f"{name}: device weight {tuple(wd.shape)} for a {tuple(w.shape)} layer")
        if bool(wd[co:].any()) or bool(wd[..., ci:].any()) or bool(bd[co:].any()):
            raise Fault("fold", f"{name}: padding rows or channels are not zero")
        _held("fold", f"{name} weight", wd[:co, :, :, :ci], w, _weight_bound(w, e_w, bn is not None))
        _held("fold", f"{name} bias", bd[:co], b, e_b)


def named_modules(model):
    """(name, module, the stem pack or None) of every conv of the model: the leaves of model.modules() and the unfused heads"""
    bb = model.backbone
    out = [("backbone.conv1", bb.conv1, getattr(bb, "stem", None))]
    for si, st in enumerate(bb.stages):
        for bi, b in enumerate(st):
            out += [(f"layer{si + 1}.{bi}.{n}", getattr(b, n), None) for n in ("conv1", "conv2", "downsample") if getattr(b, n) is not None]
    out += [(f"neck.{i}", m, None) for i, m in enumerate(model.neck)]
    out += [("head1", model.head1, None), ("head2", model.head2, None)]
    out += [(f"heads.{n}.{i}", model.heads[n][i], None) for n in HEADS for i in (0, 1)]
    assert {id(m) for _, m, _ in out} >= {id(m) for m in model.modules()}, "a conv of the model is not judged"
    return out


def pack_unfused(model, device):
    """the unfused heads are no children of the model (to() does not pack them): pack them from their raw parameters"""
    for n in HEADS:
        for m in model.heads[n]:
            m.to(device)


def check_folding(model):
    for name, m, stem in named_modules(model):
        check_module_fold(m, name, stem)


def check_fused_weights(model):
    """head1 / head2 as the device holds them are the unfused heads' device weights in the order hm | wh | reg: rows [64 i, 64 i + 64) of
    head1, block (rows of head i, columns [64 i, 64 i + 64)) of head2; every other entry of head2, and its pad rows, exactly zero"""
    hc, nc = model.head_conv, model.num_classes
    w1, b1 = unpack(model.head1.packed)
    w2, b2 = unpack(model.head2.packed)
    live = torch.zeros(w2.shape[:1] + w2.shape[3:], dtype=torch.bool, device=w2.device)
    o = 0
    for i, n in enumerate(HEADS):
        (u1, ub1), (u2, ub2) = unpack(model.heads[n][0].packed), unpack(model.heads[n][1].packed)
        co = model.heads[n][1].cout
        if o != (0, nc, nc + 2)[i] or co != (nc, 2, 2)[i]:
            raise Fault("fused weights", f"{n} does not start at channel {(0, nc, nc + 2)[i]}")
        if not (torch.equal(w1[i * hc:(i + 1) * hc], u1[:hc]) and torch.equal(b1[i * hc:(i + 1) * hc], ub1[:hc])):
            raise Fault("fused weights", f"head1 rows of {n}")
        if not (torch.equal(w2[o:o + co, 0, 0, i * hc:(i + 1) * hc], u2[:co, 0, 0, :hc]) and torch.equal(b2[o:o + co], ub2[:co])):
            raise Fault("fused weights", f"head2 block of {n}")
        live[o:o + co, i * hc:(i + 1) * hc] = True
        o += co
    if bool(w2[:, 0, 0][~live].any()) or bool(b2[o:].any()):
        raise Fault("fused weights", "head2 has a non-zero entry outside its three blocks")


# ---------------------------------------------------------------------------------------------------------------------------------
# the transposed conv by its scatter definition
# ---------------------------------------------------------------------------------------------------------------------------------
def deconv_scatter(x, w, s, p):
    """x [n, h, w, cin], w [cin, cout, k, k] float64 -> y [n, (h - 1) s - 2 p + k, (w - 1) s - 2 p + k, cout]:
    y[n, iy s - p + ky, ix s - p + kx, co] += x[n, iy, ix, ci] w[ci, co, ky, kx], contributions outside y dropped"""
    n, h, wd, _ = x.shape
    k = w.shape[2]
    full = torch.zeros((n, (h - 1) * s + k, (wd - 1) * s + k, w.shape[1]), dtype=torch.float64, device=x.device)
    for ky in range(k):
        for kx in range(k):
            full[:, ky:ky + (h - 1) * s + 1:s, kx:kx + (wd - 1) * s + 1:s] += x @ w[:, :, ky, kx]
    return full[:, p:full.shape[1] - p, p:full.shape[2] - p].contiguous()


def deconv_stage(x, e_x, w, bias, s, p, relu):
    """cc.conv_stage for a transposed conv: (exact float64 y, bound); e_x None: exact-regime data -> (the bf16 result, None)"""
    k, cin = w.shape[2], w.shape[0]
    pre = deconv_scatter(x.double(), w, s, p) + bias.double()
    if e_x is None:
        return cc.epilogue(pre, relu), None
    if torch.is_tensor(e_x):
        prop = deconv_scatter(e_x, w.abs(), s, p)
        absum = deconv_scatter(x.double().abs() + e_x, w.abs(), s, p) + bias.double().abs()
    else:
        prop, absum = 0.0, deconv_scatter(x.double().abs(), w.abs(), s, p) + bias.double().abs()
    return cc.gaussian_bound(pre, absum, cc.accumulation_c((-(-k // s)) ** 2 * cin + 1), relu, None, prop)


# ---------------------------------------------------------------------------------------------------------------------------------
# DCNv2 in the chain
# ---------------------------------------------------------------------------------------------------------------------------------
def _adjacent(z):
    """per (image, channel): the largest difference of vertically / horizontally adjacent pixels of the zero-extended image"""
    zp = torch.nn.functional.pad(z, (0, 0, 1, 1, 1, 1))
    return (zp[:, 1:] - zp[:, :-1]).abs().amax((1, 2)), (zp[:, :, 1:] - zp[:, :, :-1]).abs().amax((1, 2))


def dcn_exact(x, off, k, stride, pad, yx=True):
    """the published DCNv2 columns in float64 at float64 coordinates (the definition sc.deform_cols states, without its fp32 steps):
    -> (samples [N, Ho, Wo, k k, C], mask [N, Ho, Wo, k k], (y, x, logit) [N, Ho, Wo, k k]); a column is sample * mask"""
    N, H, W, C = x.shape
    _, Ho, Wo, _ = off.shape
    T, dev = k * k, x.device
    t = torch.arange(T, device=dev)
    by = (torch.arange(Ho, device=dev) * stride - pad)[:, None, None] + (t // k)[None, None, :]
    bx = (torch.arange(Wo, device=dev) * stride - pad)[None, :, None] + (t % k)[None, None, :]
    a, b = (0, 1) if yx else (1, 0)
    y, xx, l = by[None] + off[..., a:2 * T:2], bx[None] + off[..., b:2 * T:2], off[..., 2 * T:3 * T]
    ok = sc.in_range(y, xx, H, W)
    z = torch.zeros_like(y)
    ys, xs = torch.where(ok, y, z), torch.where(ok, xx, z)
    px, _ = sc._corners(x, torch.arange(N, device=dev).view(N, 1, 1, 1), ys, xs, ok)
    ly, lx = (ys - torch.floor(ys))[..., None], (xs - torch.floor(xs))[..., None]
    acc = (1 - ly) * (1 - lx) * px[0] + (1 - ly) * lx * px[1] + ly * (1 - lx) * px[2] + ly * lx * px[3]
    return acc, 1.0 / (1.0 + torch.exp(-l)), (y, xx, l)


def dcn_chain(x, e_x, off, e_off, k, stride, pad):
    """the columns of the chain: exact values x (bound e_x) sampled at the exact offsets off (bound e_off) -> (cols, bound on the device's
    bf16 columns); the module docstring derives every term"""
    N, H, W, C = x.shape
    T = k * k
    acc, m, (y, xx, l) = dcn_exact(x, off, k, stride, pad)
    cols = acc * m[..., None]
    e_x = e_x if torch.is_tensor(e_x) else torch.full_like(x, e_x)
    e_off = e_off if torch.is_tensor(e_off) else torch.full_like(off, e_off)
    # coordinates: fl(base + off') against base + off: the offset's bound, then one fp32 add of values below |c| + e + 1
    ecy = e_off[..., 0:2 * T:2] + 2 * U * (y.abs() + e_off[..., 0:2 * T:2] + 1)
    ecx = e_off[..., 1:2 * T:2] + 2 * U * (xx.abs() + e_off[..., 1:2 * T:2] + 1)
    e_l = e_off[..., 2 * T:3 * T]
    Ly, Lx = _adjacent(x)                                                                   # [N, C]
    big = (x.abs() + e_x).amax((1, 2))[:, None, None, None, :]
    move = torch.minimum(ecy[..., None] * Ly[:, None, None, None, :] + ecx[..., None] * Lx[:, None, None, None, :],
                         2 * x.abs().amax((1, 2))[:, None, None, None, :])
    e_acc = e_x.amax((1, 2))[:, None, None, None, :] + move + sc.SAMPLE * big + sc.TINY
    e_m = torch.clamp(e_l / 4 + 2.0 * (2.0 * (l.abs() + e_l) + 4.0) * U + sc.TINY, max=1.0)[..., None]
    e = acc.abs() * e_m + m[..., None] * e_acc + e_acc * e_m
    e = e + sc.RND * (cols.abs() + e) + sc.TINY                                             # the fp32 product acc * m
    e = e + cc.bf16_quantum(cols.abs() + e) / 2
    shape = (N, off.shape[1], off.shape[2], T * C)
    return cols.reshape(shape), e.reshape(shape)


# ---------------------------------------------------------------------------------------------------------------------------------
# the judge
# ---------------------------------------------------------------------------------------------------------------------------------
class Launches:
    """the worst err / bound per kind of launch; a launch past its bound is a Fault('launch', ...)"""

    def __init__(self):
        self.by_kind = {}
        self.trace = None             # judge(raw=True): (kind, module, input, residual, relu, output) of every layer of the restatement

    def held(self, kind, where, got, want, bound):
        err = (got.double() - want).abs()
        r = err / bound
        worst = float(torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf"))).max())
        self.by_kind[kind] = max(self.by_kind.get(kind, 0.0), worst)
        if not worst <= 1.0:
            raise Fault("launch", f"{kind} at {where}: worst err / bound {worst:.3f}, {int((r > 1).sum())} of {r.numel()} outputs past it")

    def same(self, kind, where, got, want_bits):
        self.by_kind.setdefault(kind, 0.0)
        bad = _bits(got) != want_bits
        if bool(bad.any()):
            raise Fault("launch", f"{kind} at {where}: {int(bad.sum())} of {bad.numel()} outputs differ")


def _raw(weight, bias, bn, device):
    """the float64 fold itself as logical weights: the restatement with the weights' bf16 rounding switched off"""
    w, b, _, _ = fold64(weight, bias, bn)
    return w.permute(0, 2, 3, 1).contiguous().to(device), b.to(device)


def _conv(L, kind, where, m, t, e, td, relu, res=None, launch=True, raw=False):
    """one ConvModule: alone on the device's input (+ the device's residual) against cc.conv_stage, and appended to the chain.
    res = (chain value, chain bound, device tensor) of the residual -> (t, e, td)"""
    wl, b = _raw(m.weight, m.bias, m.bn, t.device) if raw else unpack(m.packed)
    t = t[..., :wl.shape[3]]
    n, h, w, _ = t.shape
    geo = cc._plain(n, h, w, wl.shape[3], m.k, m.stride, m.pad, wl.shape[0])
    yd = None
    if launch:
        yd = m(td) if res is None else m(td, residual=res[2])
        want, bound = cc.conv_stage(td.double(), 0.0, wl, b, geo, relu, None if res is None else res[2].double())
        L.held(kind, where, yd, want, bound)
    if res is None:
        y, ey = cc.conv_stage(t, e, wl, b, geo, relu)
    else:
        y, ey = cc.conv_stage(t, e, wl, b, geo, relu, res[0], res[1])
    if L.trace is not None:
        L.trace.append(("conv", m, t, None if res is None else res[0], relu, y))
    return y, ey, yd


def _dcn(L, where, m, t, e, td, launch=True, raw=False):
    """one DeformConvModule: its three launches each on the device's input of that launch (offset conv / md_deform_cols / the K = 9 C
    GEMM), the module's own call bit for bit their result, and the chain through dcn_chain"""
    from minddet_amd import _lib, nn_ops

    wo, bo = _raw(m.offset_weight, m.offset_bias, None, t.device) if raw else unpack(m.packed_offset)
    wl, b = _raw(m.weight, m.bias, m.bn, t.device) if raw else unpack(m.packed)
    n, h, w, c = t.shape
    k, T = m.k, m.k * m.k
    geo = cc._plain(n, h, w, c, k, m.stride, m.pad, wo.shape[0])
    ho, wo_ = geo.sub_h, geo.sub_w
    w2 = wl.reshape(wl.shape[0], 1, 1, T * c)                                               # K order 0: (tap, channel), the columns' order
    geo2 = cc._plain(n, ho, wo_, T * c, 1, 1, 0, wl.shape[0])
    yd = None
    if launch:
        offd = nn_ops.conv2d(td, m.packed_offset)
        L.held("dcn offset conv", where, offd, *cc.conv_stage(td.double(), 0.0, wo, bo, geo, 0))
        colsd = torch.empty((n, ho, wo_, T * c), dtype=torch.bfloat16, device=td.device)
        _lib.call("md_deform_cols", [td, offd, colsd], extra=nn_ops._PoolAttrs3(k, m.stride, m.pad, 0))
        nb, worst, first = sc.check(colsd, *sc.deform_cols(td, offd, k, m.stride, m.pad))
        L.by_kind["md_deform_cols"] = max(L.by_kind.get("md_deform_cols", 0.0), worst)
        if nb:
            raise Fault("launch", f"md_deform_cols at {where}: {nb} of {colsd.numel()} columns outside sample_contract; first at {first}")
        pw = nn_ops.PackedConv(m.packed.w, m.packed.bias, T * c, m.packed.cout, 1, 1, 1, 0, m.packed.relu)
        pw.cin_real, pw.korder = T * c, 0
        yd = nn_ops.conv2d(colsd, pw)
        L.held("dcn GEMM K=9C", where, yd, *cc.conv_stage(colsd.double(), 0.0, w2, b, geo2, 1))
        L.same("dcn module == its launches", where, m(td), _bits(yd))
    off, e_off = cc.conv_stage(t, e, wo, bo, geo, 0)
    cols, e_cols = dcn_chain(t, e, off, e_off, k, m.stride, m.pad)
    y, ey = cc.conv_stage(cols, e_cols, w2, b, geo2, 1)
    if L.trace is not None:
        L.trace.append(("dcn", m, t, None, 1, y))
    return y, ey, yd


def _deconv(L, where, m, t, e, td, launch=True, raw=False):
    if raw:
        wd, b = _raw(m.weight_t.permute(1, 0, 2, 3), None, m.bn, t.device)                    # [cout, k, k, cin]
        wd = wd.permute(3, 0, 1, 2)
    else:
        wd, b = deconv_logical(m.packed, m.pad)
    yd = None
    if launch:
        yd = m(td)
        L.held(f"deconv k{m.k} s{m.stride} p{m.pad}", where, yd, *deconv_stage(td.double(), 0.0, wd, b, m.stride, m.pad, int(m.relu)))
    y, ey = deconv_stage(t, e, wd, b, m.stride, m.pad, int(m.relu))
    if L.trace is not None:
        L.trace.append(("deconv", m, t, None, int(m.relu), y))
    return y, ey, yd


def judge(model, images, launch=True, raw=False):
    """model on its device with the unfused heads packed (pack_unfused); images: the [N, H, W, 8] layout or the stem layout.
    -> dict(head: the device head tensor rebuilt from the single launches (None without launches), neck: the device neck output,
    value / bound: the chain's [N, H/4, W/4, nc + 4] float64, launches: worst err / bound per kind, chain: worst chain ratio)"""
    from minddet_amd import nn_ops

    assert not (raw and launch), "raw = the restatement alone, on the float64 fold instead of the device's bf16 weights"
    L = Launches()
    L.trace = [] if raw else None
    bb, nc, hc = model.backbone, model.num_classes, model.head_conv
    # stem
    if images.shape[3] == 4:
        wl, b = stem_logical(bb.stem)
        t, e = cc.reference_stem_pool(images, wl, b, exact=False)
        td = None
        if launch:
            td = nn_ops.stem_pool(images, bb.stem)
            L.held("md_stem_pool", "stem", td, t, e)
    else:
        t, e, yd = _conv(L, "conv 7x7 s2", "stem", bb.conv1, images.double(), 0.0, images, 1, launch=launch, raw=raw)
        td = None
        if launch:
            td = nn_ops.maxpool2d(yd, 3, 2, 1, zero_pad=True)
            L.same("maxpool 3x3 s2", "stem", td, _as_bits(cc.max_pool(yd.double())))
        if L.trace is not None:
            L.trace.append(("pool", None, t, None, 0, cc.max_pool(t)))
        t, e = cc.max_pool(t), cc.max_pool(e)
    # the four stages
    for si, st in enumerate(bb.stages):
        for bi, blk in enumerate(st):
            where = f"layer{si + 1}.{bi}"
            res = (t, e, td)
            if blk.downsample is not None:
                res = _conv(L, f"conv 1x1 s{blk.downsample.stride} downsample", where, blk.downsample, t, e, td, 0, launch=launch, raw=raw)
            u, eu, ud = _conv(L, f"conv 3x3 s{blk.conv1.stride}", where + ".conv1", blk.conv1, t, e, td, 1, launch=launch, raw=raw)
            t, e, td = _conv(L, "conv 3x3 s1 + residual", where + ".conv2", blk.conv2, u, eu, ud, 1, res=res, launch=launch, raw=raw)
    # the neck
    for i, m in enumerate(model.neck):
        where = f"neck.{i}"
        if hasattr(m, "weight_t"):
            t, e, td = _deconv(L, where, m, t, e, td, launch, raw)
        elif hasattr(m, "offset_weight"):
            t, e, td = _dcn(L, where, m, t, e, td, launch, raw)
        else:
            t, e, td = _conv(L, "conv 3x3 s1", where, m, t, e, td, 1, launch=launch, raw=raw)
    # the three unfused heads, hm | wh | reg
    vals, bnds, devs = [], [], []
    for n in HEADS:
        c1, c2 = model.heads[n]
        u, eu, ud = _conv(L, "head 3x3", f"heads.{n}.0", c1, t, e, td, 1, launch=launch, raw=raw)
        v, ev, vd = _conv(L, "head 1x1", f"heads.{n}.1", c2, u[..., :hc], eu[..., :hc] if torch.is_tensor(eu) else eu, ud, 0, launch=launch, raw=raw)
        vals.append(v[..., :c2.cout])
        bnds.append(ev[..., :c2.cout])
        devs.append(vd[..., :c2.cout] if launch else None)
    value, bound = torch.cat(vals, 3), torch.cat(bnds, 3)
    out = dict(value=value, bound=bound, neck=td, head=None, launches=L.by_kind, chain=None, trace=L.trace)
    if not launch:
        return out
    # the fused heads on the device's neck output: each launch alone, then slice by slice the unfused heads
    h1, _, h1d = _conv(L, "head1 (fused 3x3)", "head1", model.head1, td.double(), 0.0, td, 1)
    _, _, h2d = _conv(L, "head2 (fused 1x1)", "head2", model.head2, h1d.double(), 0.0, h1d, 0)
    o = 0
    for n, vd in zip(HEADS, devs):
        if not torch.equal(_bits(h2d[..., o:o + vd.shape[3]]), _bits(vd)):
            bad = _bits(h2d[..., o:o + vd.shape[3]]) != _bits(vd)
            raise Fault("fused==unfused", f"{n}: {int(bad.sum())} of {bad.numel()} outputs of head2(head1(x)) differ from the unfused head's")
        o += vd.shape[3]
    if o != nc + 4 or bool((_bits(h2d[..., o:]) != 0).any()):
        raise Fault("fused==unfused", f"the pad channels [{o}, {h2d.shape[3]}) are not exact zeros")
    # the model's own plumbing against the judge's
    head = model.features(images)
    if not torch.equal(_bits(head), _bits(h2d)):
        bad = _bits(head) != _bits(h2d)
        raise Fault("features==launches", f"{int(bad.sum())} of {bad.numel()} outputs of model.features differ from the single launches")
    r = (head[..., :nc + 4].double() - value).abs() / bound
    out.update(head=head, chain=float(r.max()))
    if not out["chain"] <= 1.0:
        raise Fault("chain", f"worst err / bound {out['chain']:.3f}; per head " +
                    ", ".join(f"{n} {float(r[..., a:b_].max()):.3f}" for n, a, b_ in zip(HEADS, (0, nc, nc + 2), (nc, nc + 2, nc + 4))))
    return out


def check_all(model, images):
    """folding, fused weights, launch by launch, fused == unfused, features == launches and the chain -> judge's dict"""
    pack_unfused(model, images.device)
    check_folding(model)
    check_fused_weights(model)
    return judge(model, images)


def report(what, out):
    print(f"{what}: chain worst err/bound {out['chain']:.3e}; launches " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(out["launches"].items())))


# ---------------------------------------------------------------------------------------------------------------------------------
# nn_ops.conv_transpose2d on its own
# ---------------------------------------------------------------------------------------------------------------------------------
class _Deconv:
    """what check_module_fold reads of a DeconvModule, around a bare nn_ops.PackedConvT"""

    def __init__(self, pct, weight_t, bn, pad):
        self.packed, self.weight_t, self.bn, self.pad = pct, weight_t, bn, pad


def check_conv_transpose(pct, weight_t, bn, pad, x, exact, extra_c=40, c_off=8):
    """nn_ops.conv_transpose2d(x, pct) through the scatter definition: the pack against the float64 fold, then the launches twice --
    into a fresh output (exact: bit for bit deconv_stage's bf16 result; else err / bound <= 1 of its gaussian bound) and into channels
    [c_off, c_off + cout) of a NaN-sentinel [.., cout + extra_c] tensor with guard zones: the slice is the fresh result bit for bit, so
    every pixel of it is written, and no other element changes.  -> worst err / bound (0.0 in the exact regime)"""
    from minddet_amd import nn_ops
    from tests.conv_checks import SENTINEL, check, check_guards, sentinel_out

    check_module_fold(_Deconv(pct, weight_t, bn, pad), f"conv_transpose k{pct.k} s{pct.stride} p{pad}")
    wd, b = deconv_logical(pct, pad)
    s, cout = pct.stride, pct.subs[0][0].cout
    n, h, w, _ = x.shape
    y = nn_ops.conv_transpose2d(x, pct)
    assert tuple(y.shape) == (n, (h - 1) * s - 2 * pad + pct.k, (w - 1) * s - 2 * pad + pct.k, cout) == (n, h * s, w * s, cout)
    ref = deconv_stage(x.double(), None if exact else 0.0, wd, b, s, pad, int(pct.relu))
    worst = check(y, ref[0] if exact else ref, exact)
    out, flat = sentinel_out((n, h * s, w * s, cout + extra_c), x.device)
    nn_ops.conv_transpose2d(x, pct, out=out, c_off=c_off)
    if x.is_cuda:
        torch.cuda.synchronize()
    check_guards(flat)
    oi = out.view(torch.int16)
    assert not bool((_bits(y) == SENTINEL).any())
    assert torch.equal(oi[..., c_off:c_off + cout], _bits(y)), "the channel slice differs from the fresh output"
    assert bool((oi[..., :c_off] == SENTINEL).all()) and bool((oi[..., c_off + cout:] == SENTINEL).all()), "a channel outside the slice changed"
    return worst
