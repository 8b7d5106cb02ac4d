"""The conv family's contract (include/minddet_hip.h) written out in plain torch: the launch-plan structs and md_conv_plan wrapper, a
weight packer, and a float64 reference of md_conv2d / md_conv2d_head / md_conv1x1_dual / md_conv2d_grouped that rounds to bf16 exactly
where the header says the kernels do.  Shared by tests/test_conv_plan_cpu.py (plans), tests/test_conv_reference_cpu.py (the reference
against F.conv2d / F.conv_transpose2d composed by hand), tests/test_conv_production_gpu.py (every production call against the reference),
tests/neck_checks.py (an RPN neck layer by layer), tests/test_centerpoint_conv_gpu.py (the grouped op, CenterHead and CenterPoint's neck),
tests/test_c3pair_gpu.py (md_c3_pair) and tests/test_pw_chain_gpu.py (md_pw_chain).

A call's arguments are (op, shapes, attrs): the shapes of its parameters in the op's order (None = NULL) and its attribute record as a
dict with the field names of md_conv2d_attrs / md_conv1x1_dual_attrs -- the form tests/golden/conv_plans.json stores."""
import ctypes
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from minddet_amd import _lib, nn_ops

IGEMM, PINGPONG, STREAM, HALO = 1, 2, 3, 4
ATTR_CLS = {"md_conv2d": nn_ops._ConvAttrs, "md_conv2d_head": nn_ops._ConvAttrs, "md_conv1x1_dual": nn_ops._DualAttrs}


class Launch(ctypes.Structure):   # md_conv_launch (include/minddet_hip.h)
    _fields_ = [(n, ctypes.c_int32) for n in (
        "family", "kernel_id", "ct", "pt", "mode", "gen", "dual", "mf", "head", "pers", "halo", "abl", "k", "cb", "nw", "res", "silu",
        "one_halo", "single_buf", "sub", "n0", "nn", "block", "lds")] + [("grid", ctypes.c_int64)]


def kernel_name(r):
    """the demangled template instance a record names (as a kernel trace prints it)"""
    b = lambda v: "true" if v else "false"
    if r.family == IGEMM:
        wc, fc = (2, 2) if r.ct == 128 else (1, 2 if r.ct == 64 else 1)
        return f"conv_igemm_kernel<256, {wc}, {4 // wc}, {fc}, 2, {r.mode}, {r.gen}, {r.dual}>"
    if r.family == PINGPONG:
        return f"conv_pingpong_kernel<{r.abl}, {r.mf}, {r.gen}, {b(r.head)}, {b(r.pers)}, {b(r.halo)}>"
    if r.family == STREAM:
        return f"conv1x1_stream_kernel<{r.k}, {r.cb}, {b(r.silu)}, {r.res}, {r.nw}>"
    assert r.family == HALO
    return f"conv3x3_halo_kernel<{r.ct}, {b(r.one_halo)}>"


def _struct(cls, d):
    s = cls()
    for k, v in d.items():
        setattr(s, k, _struct(type(getattr(s, k)), v) if isinstance(v, dict) else v)
    return s


def plan(op, shapes, attrs, dtypes=None, lib_path=None):
    """-> (rc, [Launch]).  Tensor pointers are fake non-null addresses: the plan never dereferences them."""
    lib = ctypes.CDLL(lib_path or _lib.LIB_PATH)
    n = len(shapes)
    params = (ctypes.c_void_p * n)(*[None if s is None else 0x100000 * (i + 1) for i, s in enumerate(shapes)])
    ndims = (ctypes.c_int * n)(*[0 if s is None else len(s) for s in shapes])
    bufs = [(ctypes.c_int64 * max(len(s or []), 1))(*(s or [0])) for s in shapes]
    shp = (ctypes.POINTER(ctypes.c_int64) * n)(*[ctypes.cast(b_, ctypes.POINTER(ctypes.c_int64)) for b_ in bufs])
    dts = (ctypes.c_char_p * n)(*[None if d is None else d.encode() for d in (dtypes or [None] * n)])
    cnt = ctypes.c_int(0)
    out = (Launch * 64)()
    rc = lib.md_conv_plan(op.encode(), n, params, ndims, shp, dts, ctypes.byref(attrs), out, 64, ctypes.byref(cnt))
    assert cnt.value <= 64
    return rc, [out[i] for i in range(cnt.value)]


def conv_attrs(kh, stride=1, pad=0, relu=0, **kw):
    """an md_conv2d_attrs record as a dict (every field present, tune all zero) -- square kernel"""
    d = {f: 0 for f, _ in nn_ops._ConvAttrs._fields_ if f != "tune"}
    d.update(kh=kh, kw=kh, stride=stride, pad=pad, relu=relu, **kw)
    d["tune"] = {f: 0 for f, _ in nn_ops.ConvTune._fields_}
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry: what one md_conv2d call reads and writes (md_conv2d_attrs in the header)
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Geometry:
    kh: int
    kw: int
    stride: int
    pad_top: int
    pad_left: int
    sub_h: int            # output rows / cols the call computes
    sub_w: int
    out_stride: int
    off_y: int
    off_x: int
    c_off: int            # first output channel written
    cout: int
    x_c_off: int          # first input channel read
    cin: int
    y_shape: tuple        # the full output tensor [N, Hf, Wf, Ctot]

    @property
    def k(self):
        return self.kh * self.kw * self.cin


def conv_geometry(shapes, a):
    """md_conv2d / md_conv2d_head: shapes[0] = x, shapes[-1] = the output"""
    n, h, w, c = shapes[0]
    y = tuple(shapes[-1])
    kh, kw, s = a["kh"], a["kw"], a["stride"]
    cin, xc0 = (a["x_cin"], a["x_c_off"]) if a["x_cin"] else (c, 0)
    if a["adv"]:
        return Geometry(kh, kw, s, a["pad_top"], a["pad_left"], a["sub_h"], a["sub_w"], a["out_stride"], a["out_off_y"], a["out_off_x"],
                        a["c_off"], a["cout"], xc0, cin, y)
    p = a["pad"]
    ho, wo = (h + 2 * p - kh) // s + 1, (w + 2 * p - kw) // s + 1
    cout = 256 if len(shapes) == 6 else y[3]   # the head op's first conv has 256 output channels
    return Geometry(kh, kw, s, p, p, ho, wo, 1, 0, 0, 0, cout, xc0, cin, y)


def out_view(y, g):
    """the elements of y (any [N, Hf, Wf, Ctot] tensor) one call writes, as an [N, sub_h, sub_w, cout] view"""
    return y[:, g.off_y:g.off_y + (g.sub_h - 1) * g.out_stride + 1:g.out_stride,
             g.off_x:g.off_x + (g.sub_w - 1) * g.out_stride + 1:g.out_stride, g.c_off:g.c_off + g.cout]


def written_mask(g, device="cpu"):
    """[Hf, Wf, Ctot] bool: True where the call writes (the same for every image)"""
    m = torch.zeros(g.y_shape[1:], dtype=torch.bool, device=device)
    out_view(m[None], g)[...] = True
    return m


def pack_weight(wl, korder, kpad, cout_pad):
    """logical weight [cout, kh, kw, cin] -> the packed [cout_pad, kpad] operand of the header: K order 0 = (kh, kw, ci),
    1 = (ci / 64, kh, kw, ci % 64); K zero padded to kpad and Cout to cout_pad.  Keeps wl's dtype."""
    cout, kh, kw, cin = wl.shape
    if korder == 1:
        assert cin % 64 == 0
        wl = wl.reshape(cout, kh, kw, cin // 64, 64).permute(0, 3, 1, 2, 4)
    wp = torch.zeros((cout_pad, kpad), dtype=wl.dtype, device=wl.device)
    wp[:cout, :kh * kw * cin] = wl.reshape(cout, -1)
    return wp


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------------------
def conv_sum(x, wl, g, absolute=False):
    """float64 [n, sub_h, sub_w, cout]: sum over taps and channels of x[n, ho*stride - pad_top + i, wo*stride - pad_left + j,
    x_c_off + ci] * wl[c, i, j, ci] (zero outside x) -- an explicit tap loop of float64 GEMMs.  absolute: sum of |x * w| instead."""
    xs = x[..., g.x_c_off:g.x_c_off + g.cin].double()
    w = wl.double()
    if absolute:
        xs, w = xs.abs(), w.abs()
    n, h, wd, _ = xs.shape
    pb = (g.sub_h - 1) * g.stride + g.kh - g.pad_top - h     # rows / cols past the input the last output reads (< 0: unread)
    pr = (g.sub_w - 1) * g.stride + g.kw - g.pad_left - wd
    xp = F.pad(xs, (0, 0, g.pad_left, pr, g.pad_top, pb))
    acc = torch.zeros((n * g.sub_h * g.sub_w, g.cout), dtype=torch.float64, device=x.device)
    for i in range(g.kh):
        for j in range(g.kw):
            tap = xp[:, i:i + (g.sub_h - 1) * g.stride + 1:g.stride, j:j + (g.sub_w - 1) * g.stride + 1:g.stride]
            acc.addmm_(tap.reshape(-1, g.cin), w[:, i, j, :].t())
    return acc.view(n, g.sub_h, g.sub_w, g.cout)


def dual_sum(xa, xb, wl, stride_b, absolute=False):
    """md_conv1x1_dual: float64 wl . [x_a ; x_b sampled with stride_b] over [n, Ho, Wo, cout]; wl [cout, Ca + Cb]"""
    a, b, w = xa.double(), xb[:, ::stride_b, ::stride_b].double(), wl.double()
    if absolute:
        a, b, w = a.abs(), b.abs(), w.abs()
    ca = a.shape[3]
    return a @ w[:, :ca].t() + b @ w[:, ca:].t()


def residual_values(r, a, g):
    """float64 residual at each output element [n, sub_h, sub_w, cout] of md_conv2d (r: the residual tensor of those images)"""
    if r is None:
        return None
    if a["res_slice"]:
        r = r[..., a["res_c_off"]:a["res_c_off"] + g.cout]
    elif a["res_upsample"]:
        r = r.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :g.sub_h, :g.sub_w]
    else:
        assert not a["adv"], "a whole-tensor residual with generalised addressing is outside the header's contract"
    return r.double()


def reference_conv2d(x, wl, bias, r, shapes, a):
    """md_conv2d's whole output for exact-regime data (where SiLU is rounded as float64): the float64 value of every element the call
    writes, NaN elsewhere, in the output's [N, Hf, Wf, Ctot] layout"""
    g = conv_geometry(shapes, a)
    y = torch.full(tuple(shapes[-1]), float("nan"), dtype=torch.float64, device=x.device)
    pre = conv_sum(x, wl, g) + bias[:g.cout].double()
    out_view(y, g)[...] = epilogue(pre, a["relu"], residual_values(r, a, g))
    return y


def bf16_quantum(v):
    """float64 spacing of bf16 numbers at |v| (8 significant bits; subnormal spacing 2^-133)"""
    e = torch.frexp(v.abs())[1].to(torch.float64)   # |v| in [2^(e-1), 2^e)
    return torch.exp2(torch.clamp(e - 8, min=-133))


def bf16_rne(v):
    """float64 -> the nearest bf16 value, ties to even, as float64 -- ONE rounding (a float64 -> bf16 cast may round twice,
    through fp32).  Finite inputs below the bf16 overflow threshold."""
    q = bf16_quantum(v)
    return torch.round(v / q) * q      # torch.round: half to even; v / q and the product are exact (q a power of two)


def silu64(v):
    return v / (1.0 + torch.exp(-v))


def act64(v, relu):
    """md_conv2d_attrs.relu in float64; ReLU gives +0.0 for v <= 0 (the kernels' v_pk_max_i16 / fmaxf do)"""
    if relu == 1:
        return torch.where(v > 0, v, torch.zeros((), dtype=v.dtype, device=v.device))
    return silu64(v) if relu == 2 else v


def epilogue(pre, relu, res=None, t=None):
    """The kernels' rounding points (conv.hip epilogues): t = bf16(act(conv + bias)) -- ReLU deferred past the residual -- then, with a
    residual, y = bf16(t + res) and ReLU.  pre: float64 conv + bias; res: float64 values of the bf16 residual at each output element.
    t overrides the first rounding (the SiLU ambiguity below).  Returns float64 values that are exactly bf16 numbers."""
    if res is None:
        return bf16_rne(act64(pre, relu)) if t is None else t
    t = bf16_rne(act64(pre, 2 if relu == 2 else 0)) if t is None else t
    return act64(bf16_rne(t + res), 1 if relu == 1 else 0)


def silu_delta(v):
    """Bound on the relative error of the kernels' fp32 SiLU, v * v_rcp_f32(1 + __expf(-v)), for an fp32-exact v (u = 2^-24):
    __expf(-v) is v_exp_f32(-v * log2 e): the fp32 product errs by <= u |v log2 e| (+ u |v log2 e| for the rounded constant), which
    2^t turns into a relative error <= 2 u |v| ln 2 log2 e = 2 u |v|; v_exp_f32 adds <= 1 ulp (2 u).  1 + e: <= u more.  v_rcp_f32 is
    within 1 ulp (2 u), the product v * r within u.  First order: (2 |v| + 2 + 1 + 2 + 1) u; with a factor 2 of margin for the
    second-order terms and the ulp-vs-relative slack, delta(v) = (4 |v| + 12) u."""
    return (4.0 * v.abs() + 12.0) * 2.0 ** -24


def silu_rounding(pre):
    """SiLU's first rounding with the kernels' error: (t_rne, t_other, near).  near marks the elements whose float64 SiLU lies within
    delta |s| of a bf16 rounding midpoint: there the kernel may round to t_other, the bf16 neighbour on the far side."""
    s = silu64(pre)
    q = bf16_quantum(s)
    lo = torch.floor(s / q) * q
    near = (s - (lo + q / 2)).abs() <= silu_delta(pre) * s.abs()
    t = bf16_rne(s)
    other = torch.where(t == lo, lo + q, lo)
    return t, other, near


def accumulation_c(n_terms):
    """c in the fp32 accumulation bound |acc - exact| <= c 2^-24 sum|x w| for a sum of n_terms exactly representable terms (the bf16 x
    bf16 products are exact in fp32; so is the fp32 bias): any order of the n - 1 additions errs by <= gamma_{n-1} sum|t| (Higham,
    Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4), gamma_m = m u / (1 - m u).  The unit roundoff u is 2^-24 for
    round-to-nearest adds; the MFMA datapath's internal rounding is not specified, so u = 2^-23 (directed rounding) is taken:
    c = 2 m / (1 - m 2^-23), m = n_terms."""
    m = n_terms
    return 2.0 * m / (1.0 - m * 2.0 ** -23)


def gaussian_bound(pre, abs_sum, c, relu, res=None, e_in=0.0, res_e=0.0):
    """|y - exact| bound for one conv + bias (+ act) (+ residual) output whose fp32 pre-activation errs by <= gamma = c 2^-24 abs_sum
    plus e_in (the error its inputs carry from earlier layers, propagated through |w|); res_e: the error the residual carries.
    Each rounding point adds half a bf16 ulp of the value it rounds: q(|value| + error so far) / 2.  ReLU and the identity are
    1-Lipschitz; SiLU's slope is below 1.1, and its fp32 evaluation adds silu_delta.  Returns (exact float64 y, bound)."""
    g = c * 2.0 ** -24 * abs_sum + e_in
    v = act64(pre, 2 if relu == 2 else (0 if res is not None else relu))
    e = g if relu != 2 else 1.1 * g + silu_delta(pre.abs() + g) * (v.abs() + 1.1 * g)
    e = e + bf16_quantum(v.abs() + e) / 2
    if res is None:
        return v, e
    y = v + res
    e = e + res_e
    e = e + bf16_quantum(y.abs() + e) / 2
    return act64(y, 1 if relu == 1 else 0), e


def conv_stage(x, e_x, wl, bias, g, relu, res=None, res_e=0.0):
    """one conv of a chain on inputs x (float64 exact values of bf16 tensors, or the exact values of an earlier stage) that carry the
    error bound e_x (None: exact inputs): exact-regime data -> (bf16 result as float64, None); else -> gaussian_bound's (y, bound)"""
    pre = conv_sum(x, wl, g) + bias.double()
    if e_x is None:
        return epilogue(pre, relu, res), None
    if torch.is_tensor(e_x):
        prop = conv_sum(e_x, wl, g, absolute=True)
        absum = conv_sum(x.double().abs() + e_x, wl, g, absolute=True) + bias.double().abs()
    else:
        prop, absum = 0.0, conv_sum(x, wl, g, absolute=True) + bias.double().abs()
    return gaussian_bound(pre, absum, accumulation_c(g.k + 1), relu, res, prop, res_e)


def _plain(n, h, w, cin, k, stride, pad, cout):
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    return Geometry(k, k, stride, pad, pad, ho, wo, 1, 0, 0, 0, cout, 0, cin, (n, ho, wo, cout))


def reference_head(x, wl, bias, w2l, b2, g, exact=True):
    """md_conv2d_head: y2 = bf16(b2 + w2[:16] . bf16(relu(conv(x) + b))) -> float64 y2 (exact) or (y2, bound)"""
    t, e = conv_stage(x, None if exact else 0.0, wl, bias[:256], g, 1)
    n, h, w, _ = t.shape
    y, e2 = conv_stage(t, e, w2l[:, None, None, :], b2[:16], _plain(n, h, w, 256, 1, 1, 0, 16), 0)
    return y if exact else (y, e2)


def reference_dual(xa, xb, wl, bias, stride_b, relu, exact=True):
    """md_conv1x1_dual: bf16(act(w . [x_a ; x_b[::s, ::s]] + b)) -> float64 (exact) or (y, bound)"""
    pre = dual_sum(xa, xb, wl, stride_b) + bias.double()
    if exact:
        return epilogue(pre, relu)
    absum = dual_sum(xa, xb, wl, stride_b, absolute=True) + bias.double().abs()
    return gaussian_bound(pre, absum, accumulation_c(wl.shape[1] + 1), relu)


# ---------------------------------------------------------------------------------------------------------------------------------
# md_conv2d_grouped: G narrow convs on consecutive 64-channel slices of x, each one conv_stage
# ---------------------------------------------------------------------------------------------------------------------------------
def grouped_attrs(k, couts, y_offs=None, w_rows=None, relu=0, x_c_off=0):
    """an md_conv2d_grouped_attrs record as a dict (cout / y_off / w_row as lists of G entries; default: side by side from 0)"""
    side = [sum(couts[:g]) for g in range(len(couts))]
    return dict(k=k, relu=int(relu), groups=len(couts), cin_g=64, x_c_off=x_c_off, reserved0=0, cout=list(couts),
                y_off=list(side if y_offs is None else y_offs), w_row=list(side if w_rows is None else w_rows))


def grouped_geometries(x_shape, a, y_shape=None):
    """md_conv2d_grouped: one Geometry per group -- k x k, stride 1, pad k / 2 on channels [x_c_off + 64 g, + 64) of x, written to
    channels [y_off[g], + cout[g]) of y (y_shape None: the narrowest y that holds every group)"""
    n, h, w, _ = x_shape
    k, G = a["k"], a["groups"]
    assert a["cin_g"] == 64 and k in (1, 3)
    if y_shape is None:
        y_shape = (n, h, w, (max(a["y_off"][g] + a["cout"][g] for g in range(G)) + 7) // 8 * 8)
    return [Geometry(k, k, 1, k // 2, k // 2, h, w, 1, 0, 0, a["y_off"][g], a["cout"][g], a["x_c_off"] + 64 * g, 64, tuple(y_shape))
            for g in range(G)]


def reference_grouped(x, wls, biases, a, y_shape, exact=True):
    """md_conv2d_grouped's whole output: wls[g] the logical [cout_g, k, k, 64] weight of group g, biases[g] its [cout_g] bias -> the
    float64 value of every element the call writes and NaN elsewhere, in y's [N, H, W, Cy] layout (exact-regime data); else (y, bound),
    the bound NaN where y is.  One conv_stage per group."""
    y = torch.full(tuple(y_shape), float("nan"), dtype=torch.float64, device=x.device)
    bound = None if exact else torch.full_like(y, float("nan"))
    for g, wl, b in zip(grouped_geometries(x.shape, a, y_shape), wls, biases):
        assert tuple(wl.shape) == (g.cout, g.kh, g.kw, 64) and tuple(b.shape) == (g.cout,)
        v, e = conv_stage(x, None if exact else 0.0, wl, b, g, a["relu"])
        out_view(y, g)[...] = v
        if not exact:
            out_view(bound, g)[...] = e
    return y if exact else (y, bound)


def pack_grouped(wls, biases, w_rows=None, rows=None, fill=0.0):
    """the operands of the header: w [R, k*k*64] with w[w_row[g] + c, tap * 64 + ci] = wls[g][c, ky, kx, ci] (tap = ky * k + kx), bias [R]
    f32 and w_row.  w_rows None: the groups' rows one after the other; rows no group owns hold `fill`.  Keeps the weights' dtype."""
    couts = [wl.shape[0] for wl in wls]
    if w_rows is None:
        w_rows = [sum(couts[:g]) for g in range(len(couts))]
    R = max(r + c for r, c in zip(w_rows, couts)) if rows is None else rows
    kk = wls[0].shape[1] * wls[0].shape[2] * 64
    w = torch.full((R, kk), fill, dtype=wls[0].dtype, device=wls[0].device)
    bias = torch.full((R,), fill, dtype=torch.float32, device=wls[0].device)
    for r, wl, b in zip(w_rows, wls, biases):
        for c in range(wl.shape[0]):
            for ky in range(wl.shape[1]):
                for kx in range(wl.shape[2]):
                    t = ky * wl.shape[2] + kx
                    w[r + c, t * 64:(t + 1) * 64] = wl[c, ky, kx]
            bias[r + c] = b[c]
    return w, bias, list(w_rows)


# ---------------------------------------------------------------------------------------------------------------------------------
# the fused ops (md_stem_pool, md_stem_conv, md_bottleneck): logical weights, their packing and float64 references
# ---------------------------------------------------------------------------------------------------------------------------------
STEM_LO = 7   # md_stem_layout_pad(0): the image starts at pixel (7, 7) of the stem layout


def stem_image(x4):
    """[N, H+16, W+16, 4] stem layout -> the [N, H, W, 3] image view"""
    return x4[:, STEM_LO:x4.shape[1] - 9, STEM_LO:x4.shape[2] - 9, :3]


def pack_stem_pool(wl):
    """[64, 7, 7, 3] -> w[64, 224]: K = (ky 0..6, kx 0..7, c 0..3), kx 7 and c 3 zero"""
    wp = torch.zeros((64, 7, 8, 4), dtype=wl.dtype, device=wl.device)
    wp[:, :, :7, :3] = wl
    return wp.reshape(64, 224)


def reference_stem_pool(x4, wl, bias, exact=True):
    """md_stem_pool: maxpool3x3/s2/p1(bf16(relu(conv7x7/s2/p3(image) + b))) -> [N, H/4, W/4, 64] (exact) or (y, bound).  Rounding and
    ReLU commute with the max (monotone), and the ReLU output is >= 0, so zero and -inf pool padding agree; the max of the per-element
    bounds bounds the max's error."""
    img = stem_image(x4)
    n, h, w, _ = img.shape
    y, e = conv_stage(img, None if exact else 0.0, wl, bias, _plain(n, h, w, 3, 7, 2, 3, 64), 1)
    return max_pool(y) if exact else (max_pool(y), max_pool(e))


def max_pool(t):
    """NHWC MaxPool 3x3 / s2 / p1"""
    return F.max_pool2d(t.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)


def pack_stem_conv(wl):
    """[cout, k, k, 3] (k = 6 or 3) -> w[cout, K]: K = (ky, kx', c 0..3), c 3 zero; k = 6: kx' = kx + 1 of 8, k = 3: kx' = kx of 4"""
    cout, k = wl.shape[0], wl.shape[1]
    kx, x0 = (8, 1) if k == 6 else (4, 0)
    wp = torch.zeros((cout, k, kx, 4), dtype=wl.dtype, device=wl.device)
    wp[:, :, x0:x0 + k, :3] = wl
    return wp.reshape(cout, -1)


def reference_stem_conv(x4, wl, bias, act, exact=True):
    """md_stem_conv: bf16(act(conv k/s2/p(image) + b)), p = k/2 - (k == 6) -> [N, H/2, W/2, cout]; exact: the float64 pre-activation
    (SiLU's rounding is judged by the caller, as for md_conv2d) and the geometry"""
    img = stem_image(x4)
    n, h, w, _ = img.shape
    k = wl.shape[1]
    g = _plain(n, h, w, 3, k, 2, k // 2 - (k == 6), wl.shape[0])
    if exact:
        return conv_sum(img, wl, g) + bias.double()
    return conv_stage(img, 0.0, wl, bias, g, act)


def reference_bottleneck(x, w1l, b1, w2l, b2, w3l, b3, res=None, wdl=None, bd=None, exact=True):
    """md_bottleneck: t1 = bf16(relu(conv1x1(x) + b1)), t2 = bf16(relu(conv3x3(t1) + b2)), y = relu(bf16(bf16(conv1x1(t2) + b3) + r)) with
    r = the residual tensor, else bf16(wd . x + bd) (the fused downsample conv), else x -> [N, H, W, 256] (exact) or (y, bound)"""
    n, h, w, cin = x.shape
    e0 = None if exact else 0.0
    t1, e1 = conv_stage(x, e0, w1l[:, None, None, :], b1, _plain(n, h, w, cin, 1, 1, 0, 64), 1)
    t2, e2 = conv_stage(t1, e1, w2l, b2, _plain(n, h, w, 64, 3, 1, 1, 64), 1)
    r, re = (res.double(), 0.0) if res is not None else (None, 0.0)
    if res is None and wdl is not None:
        r, re = conv_stage(x, e0, wdl[:, None, None, :], bd, _plain(n, h, w, 64, 1, 1, 0, 256), 0)
    elif res is None:
        r = x.double()
    y, e = conv_stage(t2, e2, w3l[:, None, None, :], b3, _plain(n, h, w, 64, 1, 1, 0, 256), 1, r, re)
    return y if exact else (y, e)


# ---------------------------------------------------------------------------------------------------------------------------------
# md_c3_pair and md_pw_chain: two convs in one launch, each one conv_stage
# ---------------------------------------------------------------------------------------------------------------------------------
NEAR_CAP = 2e-3   # largest share of stage-2 outputs of an exact-regime md_c3_pair draw that may take either bf16 neighbour


def grid(v):
    """the largest power of two (<= 1) that every element of v is an integer multiple of"""
    v = v.double()
    for s in range(0, 64):
        q = v * 2.0 ** s
        if bool((q == q.round()).all()):
            return 2.0 ** -s
    raise AssertionError("values are on no binary grid down to 2^-63")


def fp32_exact_bits(abs_sum, unit):
    """bits an fp32 accumulation needs to hold every partial sum of terms that are multiples of `unit` and sum to at most abs_sum in
    magnitude: below 24 the sum is exact in any summation order"""
    return float(torch.log2(abs_sum.max() / unit))


def c3_pair_weights(w1l, w2l):
    """the operands of the header from the logical weights w1l [C, C], w2l [C, 3, 3, C]: w1 [C, roundup(C, 64)] and w2 [C, roundup(9 C, 64)]
    with K order 0 (tap * C + ci) for C = 32 and 1 ((ci / 64) * 576 + tap * 64 + ci % 64) above; K zero padded"""
    c = w1l.shape[0]
    return (pack_weight(w1l[:, None, None, :], 0, (c + 63) // 64 * 64, c), pack_weight(w2l, 0 if c == 32 else 1, (9 * c + 63) // 64 * 64, c))


def reference_c3_pair(x, w1l, b1, w2l, b2, x_c_off, shortcut, exact=True):
    """md_c3_pair on channels [x_c_off, x_c_off + C) of x: t = bf16(silu(conv1x1(x) + b1)), u = bf16(silu(conv3x3/p1(t) + b2)) with the
    zero padding applied to t, y = bf16(u + x) if shortcut else u.  w1l [C, C], w2l [C, 3, 3, C] logical weights.
    exact=False -> (y, bound), the chain of two conv_stage calls.
    exact=True  -> (t, pre2, res): the stage-1 value, the float64 stage-2 pre-activation and the residual values (None without the
    shortcut); the caller judges SiLU's rounding of pre2 with silu_rounding / epilogue.  The draw has to keep the chain exact, and
    that is ASSERTED here:
      (a) no stage-1 pre-activation is `near` in silu_rounding: t is the one bf16 value every correct kernel gives;
      (b) both stages are exact in fp32 in any summation order: max(sum|t w2| + |b2|) over (the smallest bf16 quantum among the
          non-zero t times the weights' grid) is below 2^24, and likewise stage 1;
      (c) at most NEAR_CAP of the stage-2 outputs are `near` (may take either bf16 neighbour);
      (d) the shortcut add, done in fp32, rounds to the bf16 value the exact sum rounds to, for both admissible u."""
    n, h, w, _ = x.shape
    c = w1l.shape[0]
    assert tuple(w1l.shape) == (c, c) and tuple(w2l.shape) == (c, 3, 3, c)
    g1 = Geometry(1, 1, 1, 0, 0, h, w, 1, 0, 0, 0, c, x_c_off, c, (n, h, w, c))
    g2 = _plain(n, h, w, c, 3, 1, 1, c)
    xs = x[..., x_c_off:x_c_off + c].double()
    res = xs if shortcut else None
    w1 = w1l[:, None, None, :]
    if not exact:
        t, e_t = conv_stage(x, 0.0, w1, b1, g1, 2)
        return conv_stage(t, e_t, w2l, b2, g2, 2, res)
    pre1 = conv_sum(x, w1, g1) + b1.double()
    u1 = grid(xs) * grid(w1l)
    assert grid(b1) >= u1 and fp32_exact_bits(conv_sum(x, w1, g1, absolute=True) + b1.double().abs(), u1) < 24, "(b) stage 1"
    t, _, near1 = silu_rounding(pre1)
    assert not bool(near1.any()), f"(a) {int(near1.sum())} stage-1 pre-activations are near a rounding midpoint"
    u2 = float(bf16_quantum(t[t != 0]).min()) * grid(w2l)
    bits = fp32_exact_bits(conv_sum(t, w2l, g2, absolute=True) + b2.double().abs(), u2)
    assert grid(b2) >= u2 and bits < 24, f"(b) stage 2 needs {bits:.1f} bits"
    pre2 = conv_sum(t, w2l, g2) + b2.double()
    u, other, near = silu_rounding(pre2)
    share = float(near.double().mean())
    assert share <= NEAR_CAP, f"(c) either-neighbour share {share:.2e}"
    if shortcut:
        for v in (u, other):
            s = v + res
            assert torch.equal(bf16_rne(s.float().double()), bf16_rne(s)), "(d) the fp32 shortcut add changes the rounding"
    return t, pre2, res


def reference_pw_chain(t2, res, w3l, b3, w1l, b1, exact=True):
    """md_pw_chain: y = relu(bf16(bf16(conv3(t2) + b3) + res)), t1 = bf16(relu(conv1(y) + b1)); w3l [512, 128], w1l [128, 512] logical
    weights.  ReLU only, so the exact regime is exact for both outputs -> (y, t1), or ((y, e_y), (t1, e_t1))"""
    n, h, w, c = t2.shape
    cy = w3l.shape[0]
    assert tuple(w3l.shape) == (cy, c) and tuple(w1l.shape) == (c, cy) and tuple(res.shape) == (n, h, w, cy)
    y, e_y = conv_stage(t2, None if exact else 0.0, w3l[:, None, None, :], b3, _plain(n, h, w, c, 1, 1, 0, cy), 1, res.double())
    t1, e_t1 = conv_stage(y, e_y, w1l[:, None, None, :], b1, _plain(n, h, w, cy, 1, 1, 0, c), 1)
    return (y, t1) if exact else ((y, e_y), (t1, e_t1))
