"""The contract (include/minddet_hip.h) of the two kernels that sample an image at floating-point coordinates, in float64 torch:
md_deform_cols (csrc/dcn.hip, the DCNv2 im2col) and md_image_preprocess (csrc/preproc.hip, the affine warp + normalisation) -- a
reference of every output element, an elementwise bound on how far the kernel's fp32 value may lie from it before the final bf16
rounding, the acceptance rule, and the data generators of tests/test_sampling_gpu.py.  Shared with tests/test_sample_reference_cpu.py
(the references against float64 grid_sample and the numpy oracle, fp32 emulations of both kernels inside the bound, planted faults
outside it).  Pattern: tests/decode_contract.py, whose tracked values T(v, e) and operations (add, sub, mul, div: one fp32 rounding
each, charged RND = 2 u, u = 2^-24; a contraction of a * b + c into one fma rounds once instead of twice and stays inside) are used.

Sampling rule (both kernels; the same rule as grid_sample(mode='bilinear', padding_mode='zeros', align_corners=True)): the image is
extended by zeros, and the sample at (y, x) is the bilinear interpolation of the four pixels around it, (1 - ly)(1 - lx) Z[y0, x0] +
(1 - ly) lx Z[y0, x0 + 1] + ly (1 - lx) Z[y0 + 1, x0] + ly lx Z[y0 + 1, x0 + 1] with y0 = floor(y), ly = y - y0.  A coordinate in
(-1, 0) or (H - 1, H) keeps its in-image row with its partial weight.  Both kernels skip the whole sample (it is +0) unless -1 < y < H
and -1 < x < W: outside that open range all four pixels are zeros of the extension, so the value is the same; huge, infinite and NaN
coordinates fail the comparisons and never reach the conversion to int.

Exactness.  decode_contract charges every operation 2 u |result|.  Here an operation whose operands are exact (e = 0) and whose
float64 result r is an fp32 number (zero or normal) is charged nothing: the float64 result is the rounding of the true result z to 53
bits, so |z - r| is at most half a float64 ulp, far below half an fp32 ulp, and the fp32 number nearest z is r itself -- the kernel's
operation returns exactly r.  A fused a * b + c rounds the true a * b + c once; where the product is charged nothing it is the
true product, so the fused and the separate form return the same number.  Every other (inexact) operation also gets the absolute
floor TINY = 2^-126, which covers results in or below the subnormal range (relative bounds do not hold there, and a flush to zero
moves a value by less than 2^-126).  With x small integers, offsets multiples of 1/4 and mask values 0, 1/2 and 1 every operation
is exact, e = 0, and the output must equal the round-to-nearest-even bf16 of v bit for bit.

md_deform_cols.  For tap t = ky k + kx the coordinate is y = (float)(ho s - p + ky) + dy_t: one fp32 add of an exact small integer
and an exact bf16 value.  It is reproduced in torch float32 (round to nearest, as the kernel's add) and is an exact input from there
on; floor of an exact value is no decision.  ly = y - floor(y), 1 - ly, the four weight products, the four w * x products and their
sequential sum from +0 (in-image corners only, in the kernel's order) are tracked operations.
The mask is 1.0f / (1.0f + __expf(-l)).  __expf(-l) is v_exp_f32 of the fp32 product -l * log2 e (conv_contract.silu_delta's
derivation): the product errs by <= u |l log2 e| and as much again for the rounded constant, which 2^t turns into a relative error
<= 2 u |l|; v_exp_f32 adds <= 1 ulp = 2 u.  1 + E rounds once (u), the correctly rounded division once more (u); the derivative of
1 / (1 + E) with respect to E damps E's relative error by E / (1 + E) = 1 - m.  First order: ((2 |l| + 2)(1 - m) + 2) u relative;
with the factor 2 of margin e_m = 2 ((2 |l| + 2)(1 - m) + 2) u m + TINY.  Four exact cases (e_m = 0): l = 0 gives -0 * log2 e = -0,
v_exp_f32(-0) = 1, 1 + 1 = 2 and 1 / 2 = 1/2;  l >= 18 (+inf included) gives E (1 + 2^-15) < 2^-25, a quarter ulp of 1, so 1 + E
rounds to 1 and m = 1 (v is set to 1.0, the kernel's value; the float64 sigmoid is within 2^-25 of it);  l <= -89 (-inf included)
gives an fp32 product >= 128.4 > 128, v_exp_f32 returns +inf and m = 1 / inf = 0;  a NaN l gives NaN.  Between -89 and -87.3 the
quotient is subnormal (or flushed): |m| < 2^-126 there, covered by TINY.
The column is acc * m (tracked), rounded to bf16 once.  Where the range guard fails acc is +0 and the column is +0 * m = +0 for
every mask value but NaN (0 * NaN = NaN: "a NaN logit gives NaN" holds everywhere).

md_image_preprocess.  sx = m0 x + m1 y + m2 (two products and two adds of exact inputs, tracked: T(s, e_s)).  Bilinear
interpolation B of the zero-extended image is continuous and piecewise linear: inside a cell dB/dx = (1 - ly)(Z[y0, x0 + 1] -
Z[y0, x0]) + ly (Z[y0 + 1, x0 + 1] - Z[y0 + 1, x0]), at most the larger of the cell's two horizontal pixel differences.  The kernel
samples at its own fp32 coordinate s', |s' - s| <= e_s, so |B(s') - B(s)| <= e_sx Lx + e_sy Ly with Lx (Ly) the largest horizontal
(vertical) difference between adjacent pixels of the zero-extended image over the cells that meet the box s +- e_s -- a local
Lipschitz constant; floor is never a decision.  (e_s <= 1/2 is asserted where the box can meet the image, so at most 2 x 2 cells.)
The kernel's arithmetic at s' adds: lx = s' - floor(s') errs by <= u (|lx| < 1), 1 - lx by <= 2 u with its own rounding, a weight
(a product of two such factors in [0, 1]) by <= 2 u + 2 u + u = 5 u, a term w p (p an exact pixel <= P, the largest pixel of those
cells) by <= 5 u P + u P, four terms by <= 24 u P, the additions (partial sums <= P) by <= 4 u P: 28 u P, with the margin
SAMPLE = 28 RND.  Where the coordinates are exact (e_s = 0: identity, integer and quarter-pixel translations, rotations by 90
degrees) the sampling is tracked operation by operation instead, as for md_deform_cols, and is exact where every operation is.
Where the whole box lies outside (-1, Ws) x (-1, Hs), or the coordinate is not finite, the sample is exactly 0.
Then (v * (1.0f / 255.0f) - mean) / std, tracked; the black level (0 - mean) / std comes out of the same arithmetic.  Border pixels
and channels 3.. are exactly +0.

Acceptance (check): where e = 0 the output is bit for bit the round-to-nearest-even bf16 of v (a NaN where v is NaN); elsewhere it is
the RNE bf16 of some value in [v - e, v + e]: |got - v| <= e + bf16_quantum(|v| + e) / 2, as in conv_contract.gaussian_bound."""
import math

import numpy as np
import torch

from tests import decode_contract as dc
from tests.conv_contract import bf16_quantum, bf16_rne
from tests.decode_contract import RND, TINY, T, U

SAMPLE = 28 * RND        # the warp's sampling arithmetic at an inexact coordinate, per unit of the largest pixel nearby
LOGIT_ONE = 18.0         # mask logits from here up give exactly 1
LOGIT_ZERO = -89.0       # mask logits from here down give exactly 0


# ---------------------------------------------------------------------------------------------------------------------------------
# tracked operations with the exactness rule
# ---------------------------------------------------------------------------------------------------------------------------------
def _exact(r, *ops):
    """r = op(*ops) from decode_contract: no charge where every operand is exact and r.v is an fp32 number (zero or normal), else
    decode_contract's bound plus TINY"""
    rep = (r.v == r.v.float().double()) & ((r.v == 0) | (r.v.abs() >= TINY))
    for o in ops:
        if isinstance(o, T):
            rep = rep & (o.e == 0)
    return T(r.v, torch.where(rep, torch.zeros_like(r.e), r.e + TINY))


def add(a, b):
    return _exact(dc.add(a, b), a, b)


def sub(a, b):
    return _exact(dc.sub(a, b), a, b)


def mul(a, b):
    return _exact(dc.mul(a, b), a, b)


def div(a, b):
    return _exact(dc.div(a, b), a, b)


def _where(c, a, b):
    return T(torch.where(c, a.v, b.v), torch.where(c, a.e, b.e))


def _zeros(like):
    return T(torch.zeros_like(like))


def bilinear_tracked(y, x, px, inb):
    """the kernels' sampling loop at EXACT coordinates y, x (float64, any shape S; already inside the range guard): px [4, *S, C] the
    corner pixels (q = 2 qy + qx; 0 where skipped), inb [4, *S] the corners inside the image -> T [*S, C]"""
    y0, x0 = torch.floor(y), torch.floor(x)
    ly, lx = sub(T(y), T(y0)), sub(T(x), T(x0))
    one = T(torch.ones_like(y))
    hy, hx = sub(one, ly), sub(one, lx)
    acc = _zeros(px[0])
    for q in range(4):
        w = mul(ly if q >> 1 else hy, lx if q & 1 else hx)
        w = T(w.v[..., None], w.e[..., None])
        acc = _where(inb[q][..., None], add(acc, mul(w, T(px[q]))), acc)
    return acc


def _corners(img, n_idx, y, x, ok):
    """img [N, H, W, C] float64; n_idx, y, x, ok broadcastable to a shape S -> (px [4, *S, C], inb [4, *S]) of the four pixels
    around (y, x): zero and False outside the image or where ~ok"""
    N, H, W, C = img.shape
    y0, x0 = torch.floor(torch.where(ok, y, torch.zeros_like(y))).long(), torch.floor(torch.where(ok, x, torch.zeros_like(x))).long()
    flat = img.reshape(N * H * W, C)
    px, inb = [], []
    for q in range(4):
        yy, xx = y0 + (q >> 1), x0 + (q & 1)
        i = ok & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        idx = (n_idx * H + yy.clamp(0, H - 1)) * W + xx.clamp(0, W - 1)
        p = flat[idx.reshape(-1)].reshape(tuple(idx.shape) + (C,))
        px.append(torch.where(i[..., None], p, torch.zeros_like(p)))
        inb.append(i)
    return torch.stack(px), torch.stack(inb)


# ---------------------------------------------------------------------------------------------------------------------------------
# md_deform_cols
# ---------------------------------------------------------------------------------------------------------------------------------
def dcn_coords(off, H, W, k, stride, pad):
    """off [N, Ho, Wo, Coff] bf16 -> (y, x, logit) float64 [N, Ho, Wo, T]: the kernel's fp32 coordinates (exact) and mask logits"""
    _, Ho, Wo, _ = off.shape
    Tn = k * k
    dev = off.device
    o = off.float()
    t = torch.arange(Tn, device=dev)
    by = (torch.arange(Ho, device=dev) * stride - pad)[:, None, None] + (t // k)[None, None, :]
    bx = (torch.arange(Wo, device=dev) * stride - pad)[None, :, None] + (t % k)[None, None, :]
    y = by.float()[None] + o[..., 0:2 * Tn:2]          # one fp32 add each
    x = bx.float()[None] + o[..., 1:2 * Tn:2]
    return y.double(), x.double(), o[..., 2 * Tn:3 * Tn].double()


def in_range(y, x, H, W):
    """the kernels' range guard (False for NaN)"""
    return (y > -1) & (y < H) & (x > -1) & (x < W)


def mask_value(l):
    """1.0f / (1.0f + __expf(-l)) of exact logits l (float64 of bf16) -> T; see the module docstring"""
    m = 1.0 / (1.0 + torch.exp(-l))
    e = 2.0 * ((2.0 * l.abs() + 2.0) * (1.0 - m) + 2.0) * U * m + TINY
    one, zero = l >= LOGIT_ONE, l <= LOGIT_ZERO
    m = torch.where(one, torch.ones_like(m), torch.where(zero, torch.zeros_like(m), m))
    e = torch.where(one | zero | (l == 0), torch.zeros_like(e), e)
    return T(m, e)                # NaN l: v and e NaN


def deform_samples(x, off, k, stride, pad):
    """the sampling stage alone -> (T [N, Ho, Wo, T, C] of the bilinear samples, ok [N, Ho, Wo, T] the range guard)"""
    N, H, W, C = x.shape
    y, xx, _ = dcn_coords(off, H, W, k, stride, pad)
    ok = in_range(y, xx, H, W)
    n_idx = torch.arange(N, device=x.device).view(N, 1, 1, 1)
    px, inb = _corners(x.double(), n_idx, y, xx, ok)
    z = torch.zeros_like(y)
    return bilinear_tracked(torch.where(ok, y, z), torch.where(ok, xx, z), px, inb), ok


def deform_cols(x, off, k, stride, pad):
    """md_deform_cols: x [N, H, W, C] bf16, off [N, Ho, Wo, Coff >= 3 k k] bf16 -> (v, e, fill) over cols [N, Ho, Wo, k k C]; fill marks
    the elements that are exactly +0 because the range guard fails (and the logit is no NaN)"""
    N, H, W, C = x.shape
    _, Ho, Wo, _ = off.shape
    acc, ok = deform_samples(x, off, k, stride, pad)
    l = dcn_coords(off, H, W, k, stride, pad)[2]
    m = mask_value(l)
    col = mul(acc, T(m.v[..., None], m.e[..., None]))
    nan = torch.isnan(l)[..., None].expand_as(col.v)
    v = torch.where(nan, torch.full_like(col.v, math.nan), col.v)
    e = torch.where(nan, torch.zeros_like(col.e), col.e)
    fill = (~ok & ~torch.isnan(l))[..., None].expand_as(v)
    shape = (N, Ho, Wo, k * k * C)
    return v.reshape(shape), e.reshape(shape), fill.reshape(shape)


# ---------------------------------------------------------------------------------------------------------------------------------
# md_image_preprocess
# ---------------------------------------------------------------------------------------------------------------------------------
def warp_coords(mat, out_hw, device):
    """mat [N, 6] fp32 -> (sx, sy) T [N, Ho, Wo]: (m0 x + m1 y) + m2 and (m3 x + m4 y) + m5, tracked.  inf * 0 and inf - inf give NaN
    in v, as they do in fp32 in any evaluation order."""
    ho, wo = out_hw
    m = mat.double().to(device)
    ys = torch.arange(ho, dtype=torch.float64, device=device).view(1, ho, 1).expand(m.shape[0], ho, wo)
    xs = torch.arange(wo, dtype=torch.float64, device=device).view(1, 1, wo).expand(m.shape[0], ho, wo)
    c = lambda j: T(m[:, j].view(-1, 1, 1).expand_as(xs).contiguous())
    sx = add(add(mul(c(0), T(xs)), mul(c(1), T(ys))), c(2))
    sy = add(add(mul(c(3), T(xs)), mul(c(4), T(ys))), c(5))
    return sx, sy


def _cell_max(Z, n_idx, cy, cx, pad):
    """max over the listed cells (cy, cx: lists of long tensors, cell = the 2 x 2 pixels from (cy, cx)) of per-channel (Lx, Ly, P):
    the largest horizontal / vertical adjacent difference and the largest pixel.  Z [N, H + 2 pad, W + 2 pad, C] the zero-extended
    image, indices clamped into it (everything further out is zero)."""
    N, Hp, Wp, C = Z.shape
    dx = torch.zeros_like(Z)
    dx[:, :, :-1] = (Z[:, :, 1:] - Z[:, :, :-1]).abs()
    dy = torch.zeros_like(Z)
    dy[:, :-1] = (Z[:, 1:] - Z[:, :-1]).abs()
    lx = dx.clone()
    lx[:, :-1] = torch.maximum(dx[:, :-1], dx[:, 1:])                 # both rows of the cell
    ly = dy.clone()
    ly[:, :, :-1] = torch.maximum(dy[:, :, :-1], dy[:, :, 1:])        # both columns of the cell
    pm = Z.clone()
    pm[:, :-1] = torch.maximum(pm[:, :-1], Z[:, 1:])
    pm[:, :, :-1] = torch.maximum(pm[:, :, :-1], pm[:, :, 1:])
    out = None
    for yy in cy:
        for xx in cx:
            idx = ((n_idx * Hp + (yy + pad).clamp(0, Hp - 1)) * Wp + (xx + pad).clamp(0, Wp - 1)).reshape(-1)
            g = [t.reshape(N * Hp * Wp, C)[idx].reshape(tuple(yy.shape) + (C,)) for t in (lx, ly, pm)]
            out = g if out is None else [torch.maximum(a, b) for a, b in zip(out, g)]
    return out


def warp_samples(img_u8, mat, out_hw):
    """the sampling stage alone -> T [N, Ho, Wo, 3] of the bilinear samples of the zero-extended image (0 .. 255)"""
    N, Hs, Ws, _ = img_u8.shape
    dev = img_u8.device
    img = img_u8.double()
    sx, sy = warp_coords(mat, out_hw, dev)
    finite = torch.isfinite(sx.v) & torch.isfinite(sy.v) & torch.isfinite(sx.e) & torch.isfinite(sy.e)
    z = torch.zeros_like(sx.v)
    xv, yv, xe, ye = (torch.where(finite, t, z) for t in (sx.v, sy.v, sx.e, sy.e))
    out = ~finite | (xv - xe >= Ws) | (xv + xe <= -1) | (yv - ye >= Hs) | (yv + ye <= -1)        # surely outside: exactly 0
    exact = ~out & (xe == 0) & (ye == 0)
    near = ~out & ~exact
    assert not bool(near.any()) or float(torch.maximum(xe, ye)[near].max()) <= 0.5, "coordinate error above half a pixel near the image"
    n_idx = torch.arange(N, device=dev).view(N, 1, 1)
    ok = ~out & in_range(yv, xv, Hs, Ws)
    px, inb = _corners(img, n_idx, yv, xv, ok)
    tr = bilinear_tracked(torch.where(ok, yv, z), torch.where(ok, xv, z), px, inb)      # value everywhere; bound where exact
    PAD = 3
    Z = torch.nn.functional.pad(img, (0, 0, PAD, PAD, PAD, PAD))
    yn, xn, yen, xen = (torch.where(near, t, z) for t in (yv, xv, ye, xe))
    cy = [torch.floor(yn - yen).long().clamp(-PAD, Hs + PAD), torch.floor(yn + yen).long().clamp(-PAD, Hs + PAD)]
    cx = [torch.floor(xn - xen).long().clamp(-PAD, Ws + PAD), torch.floor(xn + xen).long().clamp(-PAD, Ws + PAD)]
    Lx, Ly, P = _cell_max(Z, n_idx, cy, cx, PAD)
    e_near = xe[..., None] * Lx + ye[..., None] * Ly + SAMPLE * P + TINY
    zc = torch.zeros_like(tr.v)
    v = torch.where(out[..., None], zc, tr.v)
    e = torch.where(out[..., None], zc, torch.where(exact[..., None], tr.e, e_near))
    return T(v, e)


def image_preprocess(img_u8, mat, norm, out_hw, pad_lo, pad_hi, C):
    """md_image_preprocess: img_u8 [N, Hs, Ws, 3] uint8, mat [N, 6] fp32, norm [6] fp32 (mean, std) -> (v, e, fill) over the whole padded
    output [N, pad_lo + out_h + pad_hi, pad_lo + out_w + pad_hi, C]; fill marks the border and the channels 3..: exactly +0"""
    N = img_u8.shape[0]
    ho, wo = out_hw
    dev = img_u8.device
    s = warp_samples(img_u8, mat, out_hw)
    nm = norm.double().to(dev)
    inv255 = float(np.float32(1.0) / np.float32(255.0))
    ch = lambda j: T(nm[j:j + 3].view(1, 1, 1, 3).expand_as(s.v).contiguous())
    val = div(sub(mul(s, inv255), ch(0)), ch(3))
    shape = (N, pad_lo + ho + pad_hi, pad_lo + wo + pad_hi, C)
    v = torch.zeros(shape, dtype=torch.float64, device=dev)
    e = torch.zeros_like(v)
    fill = torch.ones(shape, dtype=torch.bool, device=dev)
    v[:, pad_lo:pad_lo + ho, pad_lo:pad_lo + wo, :3] = val.v
    e[:, pad_lo:pad_lo + ho, pad_lo:pad_lo + wo, :3] = val.e
    fill[:, pad_lo:pad_lo + ho, pad_lo:pad_lo + wo, :3] = False
    return v, e, fill


# ---------------------------------------------------------------------------------------------------------------------------------
# acceptance
# ---------------------------------------------------------------------------------------------------------------------------------
def bound(v, e):
    """|got - v| allowed where e > 0: got is the RNE bf16 of a value within e of v"""
    return e + bf16_quantum(v.abs() + e) / 2


def check(got, v, e, fill_mask=None):
    """got (bf16, any device) against (v, e) -> (bad count, worst err / bound over the bounded elements, first bad index).  e == 0: bit
    for bit the RNE bf16 of v (NaN where v is NaN); e > 0: within bound(v, e) and finite; fill_mask: bit for bit +0."""
    gi = got.contiguous().view(torch.int16)
    g = got.double()
    isnan = torch.isnan(v)
    vz = torch.where(isnan, torch.zeros_like(v), v)
    ez = torch.where(isnan, torch.zeros_like(e), e)
    want = bf16_rne(vz).to(torch.bfloat16).view(torch.int16)
    exact = ez == 0
    err = (g - vz).abs()
    b = bound(vz, ez)
    ok = torch.where(isnan, torch.isnan(g), torch.where(exact, gi == want, torch.isfinite(g) & (err <= b)))
    if fill_mask is not None:
        ok = ok & (~fill_mask | (gi == 0))
    bounded = ~exact & ~isnan
    worst = 0.0
    if bool(bounded.any()):
        r = (err / b)[bounded]
        worst = float(torch.where(torch.isnan(r), torch.full_like(r, math.inf), r).max())
    bad = ~ok
    nb = int(bad.sum())
    first = tuple(int(i) for i in bad.nonzero()[0]) if nb else None
    return nb, worst, first


def e_share(got, v, e):
    """the largest share of its fp32 term e that a bounded element needs: (|got - v| - half a bf16 ulp) / e, 0 where the rounding term
    alone covers every element.  The err / bound of check sits near 1 whenever a value lands next to a bf16 tie; this figure
    compares the fp32 arithmetic of two implementations."""
    ok = (e > 0) & ~torch.isnan(v) & torch.isfinite(got.double())
    if not bool(ok.any()):
        return 0.0
    r = ((got.double() - v).abs() - bf16_quantum(v.abs() + e) / 2) / e
    return max(0.0, float(r[ok].max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------------------
DCN_SMALL_SHAPES = [(2, 5, 7), (1, 13, 21)]
DCN_SMALL_C = [8, 64]
DCN_SMALL_KSP = [(3, 1, 1), (3, 2, 1), (1, 1, 0), (4, 2, 1), (7, 1, 3)]
DCN_PRODUCTION = [(2, 16, 16, 512), (2, 32, 32, 256), (2, 64, 64, 128)]        # CenterNet-R18 neck at 512 x 512, batch 2; k 3, s 1, p 1
EXACT_LOGITS = (0.0, -120.0, 30.0, -math.inf, math.inf)                       # masks 1/2, 0, 1, 0, 1
NONFINITE_PLANTS = ((2, math.nan), (0, math.nan), (1, math.inf), (0, -math.inf), (2, math.inf), (2, -math.inf))   # (dy / dx / logit, value)
WILD_SHARE = 16                                                               # one element in 16 is a draw over every bf16 value


def dcn_small_cases():
    """[(shape, C, (k, stride, pad), Coff padded, exact regime, seed)]"""
    out = []
    for shape in DCN_SMALL_SHAPES:
        for C in DCN_SMALL_C:
            for ksp in DCN_SMALL_KSP:
                for padded in (False, True):
                    for exact in (True, False):
                        out.append((shape, C, ksp, padded, exact, 101 + len(out)))
    return out


def out_hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def coff_of(k, padded):
    return (3 * k * k + 7) // 8 * 8 if padded else 3 * k * k


def edge_targets(H, W):
    """the planted coordinates: (axis, value); axis 0 = y"""
    return ([(0, v) for v in (-1.0, 0.0, H - 1.0, float(H), -0.25, H - 0.75)] +
            [(1, v) for v in (-1.0, 0.0, W - 1.0, float(W), -0.25, W - 0.25)])


def plant_edges(off, H, W, k, stride, pad):
    """write offsets into off (float32 [N, Ho, Wo, Coff], before the bf16 cast) that put one coordinate of a tap exactly on each of
    edge_targets, the other coordinate a quarter inside the image; the last plant puts both on -1/4 (the corner cell).  Each plant
    takes the output row / column whose base position is nearest the target, so the offset stays small and the fp32 sum exact.
    Returns [(n, ho, wo, t, y, x)]: the planted taps and their coordinates."""
    N, Ho, Wo, _ = off.shape
    Tn = k * k
    taken, plants = set(), []
    base = lambda o, kk: o * stride - pad + kk
    targets = edge_targets(H, W) + [(2, -0.25)]
    for j, (axis, val) in enumerate(targets):
        t = j % Tn
        ky, kx = t // k, t % k
        n = j % N
        if axis == 0:
            ho = min(range(Ho), key=lambda o: abs(base(o, ky) - val))
            wo = j % Wo
            while (n, ho, wo, t) in taken:
                wo = (wo + 1) % Wo
            y, x = val, min(max(base(wo, kx) + 0.25, 0.25), W - 1.25)
        elif axis == 1:
            wo = min(range(Wo), key=lambda o: abs(base(o, kx) - val))
            ho = j % Ho
            while (n, ho, wo, t) in taken:
                ho = (ho + 1) % Ho
            y, x = min(max(base(ho, ky) + 0.25, 0.25), H - 1.25), val
        else:
            free = [(abs(base(h_, ky) - val) + abs(base(w_, kx) - val), h_, w_) for h_ in range(Ho) for w_ in range(Wo)
                    if (n, h_, w_, t) not in taken]
            _, ho, wo = min(free)
            y = x = val
        taken.add((n, ho, wo, t))
        dy, dx = y - base(ho, ky), x - base(wo, kx)
        assert abs(dy) <= 16 and abs(dx) <= 16       # multiples of 1/4 below 32: exact in bf16, and the sum in fp32
        off[n, ho, wo, 2 * t], off[n, ho, wo, 2 * t + 1] = dy, dx
        plants.append((n, ho, wo, t, y, x))
    return plants


def _wild_table(device):
    """every finite bf16 value, +-inf and NaN"""
    extra = torch.tensor([math.inf, -math.inf, math.nan], dtype=torch.bfloat16, device=device)
    return torch.cat([dc.all_finite_bf16(device), extra])


def gen_dcn(shape, C, k, stride, pad, padded_coff, exact, seed, device):
    """-> (x [N, H, W, C] bf16, off [N, Ho, Wo, Coff] bf16, {edges: plant_edges' list, nonfinite: [(n, ho, wo, t, kind, value)]}).
    exact: x integers |x| <= 8; offsets multiples of 1/4 in [-3, 3], dy positive and dx negative three times in four; logits from
    EXACT_LOGITS.  else: x ~ N(0, 1), offsets ~ N(0, 1.5^2), logits ~ N(0, 2^2), one element in WILD_SHARE of both replaced by a draw
    over every bf16 value (+-inf and NaN included), and NONFINITE_PLANTS on free taps near the centre.  Both: the edge plants; NaN in the channels past 3 k k."""
    N, H, W = shape
    Ho, Wo = out_hw(H, W, k, stride, pad)
    Tn, Coff = k * k, coff_of(k, padded_coff)
    g = torch.Generator(device=device).manual_seed(seed)
    rand = lambda s: torch.rand(s, generator=g, device=device)
    off = torch.empty((N, Ho, Wo, Coff), dtype=torch.float32, device=device)
    if exact:
        x = torch.randint(-8, 9, (N, H, W, C), generator=g, device=device).to(torch.bfloat16)
        mag = torch.randint(0, 13, (N, Ho, Wo, 2 * Tn), generator=g, device=device).float() / 4
        sign = torch.where(rand((N, Ho, Wo, 2 * Tn)) < 0.75, 1.0, -1.0)
        sign[..., 1::2] *= -1.0                                   # dx: mostly negative
        off[..., :2 * Tn] = mag * sign
        lv = torch.tensor(EXACT_LOGITS, device=device)
        off[..., 2 * Tn:3 * Tn] = lv[torch.randint(0, len(EXACT_LOGITS), (N, Ho, Wo, Tn), generator=g, device=device)]
    else:
        x = torch.randn((N, H, W, C), generator=g, device=device).to(torch.bfloat16)
        off[..., :2 * Tn] = torch.randn((N, Ho, Wo, 2 * Tn), generator=g, device=device) * 1.5
        off[..., 2 * Tn:3 * Tn] = torch.randn((N, Ho, Wo, Tn), generator=g, device=device) * 2.0
    off[..., 3 * Tn:] = math.nan
    ob = off.to(torch.bfloat16)
    if not exact:
        table = _wild_table(device)
        wild = rand((N, Ho, Wo, 3 * Tn)) < 1.0 / WILD_SHARE
        draw = table[torch.randint(0, table.numel(), (N, Ho, Wo, 3 * Tn), generator=g, device=device)]
        ob[..., :3 * Tn] = torch.where(wild, draw, ob[..., :3 * Tn])
    pl = torch.zeros((N, Ho, Wo, Coff), dtype=torch.float32, device="cpu")
    plants = plant_edges(pl, H, W, k, stride, pad)
    for (n, ho, wo, t, _, _) in plants:
        ob[n, ho, wo, 2 * t], ob[n, ho, wo, 2 * t + 1] = float(pl[n, ho, wo, 2 * t]), float(pl[n, ho, wo, 2 * t + 1])
        ob[n, ho, wo, 2 * Tn + t] = 0.0 if exact else 1.0         # a live mask on the planted taps
    wild_plants = []
    if not exact:                                                 # non-finite values on taps the edge plants left free, from the centre
        taken = {p[:4] for p in plants}
        free = sorted((abs(h_ - Ho // 2) + abs(w_ - Wo // 2), h_, w_, t) for h_ in range(Ho) for w_ in range(Wo) for t in range(Tn)
                      if (N - 1, h_, w_, t) not in taken)
        for (_, h_, w_, t), (ch, val) in zip(free, NONFINITE_PLANTS):
            c = 2 * Tn + t if ch == 2 else 2 * t + ch
            ob[N - 1, h_, w_, 2 * t], ob[N - 1, h_, w_, 2 * t + 1], ob[N - 1, h_, w_, 2 * Tn + t] = 0.25, 0.25, 1.0
            ob[N - 1, h_, w_, c] = val
            wild_plants.append((N - 1, h_, w_, t, ch, val))
    return x, ob, dict(edges=plants, nonfinite=wild_plants)


# --- the warp
WARP_SRC = (3, 37, 53)            # N, Hs, Ws: an odd width keeps the 3-byte pixels unaligned
WARP_OUT = (32, 64)
WARP_LAYOUTS = {"stem": (4, 7, 9), "c8": (8, 0, 0), "c8_pad35": (8, 3, 5), "c4": (4, 0, 0)}       # C, pad_lo, pad_hi
MEAN, STD = (0.408, 0.447, 0.470), (0.289, 0.274, 0.278)                                         # centernet/default_config.yaml


def _rot(deg, scale, cx_src, cy_src, cx_out, cy_out):
    """output pixel -> source pixel: rotate by deg and scale about the centres"""
    c, s = math.cos(math.radians(deg)) * scale, math.sin(math.radians(deg)) * scale
    return [c, -s, cx_src - c * cx_out + s * cy_out, s, c, cy_src - s * cx_out - c * cy_out]


def warp_matrix_sets():
    """name -> [3, 6] fp32: one matrix per image of WARP_SRC, so the batch index matters"""
    _, Hs, Ws = WARP_SRC
    ho, wo = WARP_OUT
    inf = math.inf
    sets = {
        "identity_shift": [[1, 0, 0, 0, 1, 0], [1, 0, -6, 0, 1, -3], [1, 0, 10, 0, 1, 8]],       # outside on the left, right, top; bottom
        "quarter": [[1, 0, 0.25, 0, 1, -0.75], [1, 0, -5.25, 0, 1, 6.5], [1, 0, 9.75, 0, 1, 7.25]],
        "rot90_transpose": [[0, 1, 0, -1, 0, Hs - 1], [0, 1, 0, 1, 0, 0], [0, -1, Ws - 1, 1, 0, -4]],
        "rot30_scale": [_rot(30, 1.7, Ws / 2, Hs / 2, wo / 2, ho / 2), _rot(-30, 1.7, Ws / 2, Hs / 2, wo / 2, ho / 2),
                        _rot(30, 1 / 1.7, Ws / 2, Hs / 2, wo / 2, ho / 2)],
        "scale037": [[0.37, 0, 0, 0, 0.37, 0], [0.37, 0, 11.3, 0, 0.37, -2.9], [0.37, 0, 40.1, 0, 0.37, 30.7]],
        "far": [[1, 0, 1e6, 0, 1, 0], [1e30, 0, 1e30, 0, -1e30, -1e30], [inf, 0, 0, 0, 1, -inf]],           # all black
    }
    return {k: torch.tensor(v, dtype=torch.float32) for k, v in sets.items()}


def warp_small_cases():
    """[(layout, matrix set, image kind)]: every layout x matrix set on a random image, the white and the all-zero image in the stem
    layout"""
    out = [(layout, name, "random") for layout in WARP_LAYOUTS for name in warp_matrix_sets()]
    return out + [("stem", name, kind) for kind in ("white", "zero") for name in ("identity_shift", "rot30_scale")]


def production_warp_matrices(rotate_deg):
    """[2, 6]: det_ops.get_affine_transform (output pixel -> source pixel) of a 640 x 480 image into 512 x 512, as
    tests/test_preprocess_gpu.py builds it, optionally composed with a rotation about the output centre"""
    from minddet_amd import det_ops

    mats = []
    for b in range(2):
        c = np.array([320.0 + 7 * b, 240.0 - 3 * b], np.float32)
        t = np.asarray(det_ops.get_affine_transform(c, 640.0 + 15 * b, (512, 512), inv=True), np.float64).reshape(2, 3)
        if rotate_deg:
            a = math.radians(rotate_deg)
            r = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
            ctr = np.array([[1, 0, 256], [0, 1, 256], [0, 0, 1.0]])
            t = t @ (ctr @ r @ np.linalg.inv(ctr))
        mats.append(t.reshape(6).astype(np.float32))
    return torch.from_numpy(np.stack(mats))


def gen_image(kind, shape, seed, device):
    """uint8 [N, Hs, Ws, 3]: 'random', 'white' (constant 255: the border rule at full contrast) or 'zero'"""
    if kind == "white":
        return torch.full(tuple(shape) + (3,), 255, dtype=torch.uint8, device=device)
    if kind == "zero":
        return torch.zeros(tuple(shape) + (3,), dtype=torch.uint8, device=device)
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(0, 256, tuple(shape) + (3,), generator=g, device=device, dtype=torch.uint8)


def norm_tensor(device="cpu"):
    return torch.tensor(list(MEAN) + list(STD), dtype=torch.float32, device=device)
