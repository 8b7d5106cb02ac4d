"""The two md_cn_aug_* operators (include/minddet_hip_cnaug.h) restated in vectorised numpy, with the bounds the tests hold them and the
reference to.

transform()   the random block of COCOHP.preprocess_fn and the closed form of its two matrices: float64 on the fp32 values the
              reference holds, one IEEE operation per step, in the header's order -- the device gives the same bits.
solve_bound() the closed form against the reference's own three-point solve.  u = 2^-24.  get_affine_transform builds its points in
              fp32: P0 = (cx, cy), P1 = (cx, y1) with y1 = fl(cy - s32 / 2), P2 = (fl(cx - d), y1) with d = fl(cy - y1); the dst points are
              exact for integer sizes.  The exact solve of those points is diagonal with kx = (dst_w / 2) / (cx - P2x) and
              ky = (dst_w / 2) / (cy - y1).  To first order |(cy - y1) - s32 / 2| <= u (|cy| + s32 / 2) (one rounding) and
              |(cx - P2x) - s32 / 2| <= u (|cy| + s32 / 2) + u s32 / 2 + u (|cx| + s32 / 2) (three roundings), so against k = dst_w / s32
              the relative errors are rho_y = u (|cy| + h) / h and rho_x = u (|cx| + |cy| + 3 h) / h with h = s32 / 2; the translations
              dst / 2 - k c inherit |c| |k| rho.  The reference's float64 solve (LU of a 3 x 3 system, 3 right-hand sides) adds at most
              9 x 2^-53 x cond(A) x max |M| per entry.  Second-order terms: a factor 1 + 2^-10 (rho is below 2^-10 wherever
              |c| / s32 < 2^12, which solve_bound() asserts).
sample()      the kernels' fp32 bilinear sampler (csrc/image_sample.h) as a restatement of its operation sequence, the form
              oracle/np_ops.py uses for mask pasting: fp32 products and sums, each fused multiply-add as the float64 product (exact for
              fp32 factors) plus the addend, rounded once to float64 and then to fp32 (a double rounding, which differs from the fused
              result only where the float64 sum lands within 2^-29 ulp of an fp32 tie).
colour()      the colour chain in float64 with an exactly rounded gs_mean (math.fsum), one rounding to fp32, the fp32 normalisation and
              bf16; colour_bound() is the forward bound of the reference's own fp32 operation sequence against that chain:
                grey (fp32 weights, three products, two sums of non-negative terms)       e_g <= 4 u g
                gs.mean() (numpy's pairwise fp32 sum: each term passes through at most 25 + ceil(log2(n / 128)) additions, one
                division, plus the mean of e_g)                                            e_m <= (30 + ceil(log2(n / 128))) u mean
                image *= alpha (alpha rounded to fp32, one product)                        e' = |a| e + 2 u |a x|
                blend_: image1 *= a; image2 *= 1 - a; image1 += image2                     e' = |a| e + 2 u |a x| + |1 - a| e_2 + 2 u |(1 - a) x_2| + u |x'|
                lighting_ (a float64 sum rounded once to fp32)                             e' = e + u |x'|
                (inp - mean) / std                                                         e_y = (e + u |x - mean|) / std + u |y|
              and the contract's own three roundings (x to fp32, the difference, the quotient): (u |x| + u |x - mean|) / std + u |y|.
              Magnitudes are those of the float64 chain; second-order terms: the factor 1 + 2^-10.
"""
import math

import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
f32, f64 = np.float32, np.float64
ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))     # 0 brightness_, 1 contrast_, 2 saturation_
GREY = (0.114, 0.587, 0.299)                                                    # B, G, R


# ---------------------------------------------------------------------------------------------------- md_cn_aug_transform
def transform(sizes, draws, *, rand_crop, scale, shift, flip_prop, input_hw, down_ratio):
    """sizes [B,2] (h, w), draws [B,4] f64 -> dict(c [B,2] f32 (after the flip), s [B] f64, flipped [B] bool, mat_in [B,6] f32,
    trans_out [B,6] f64, trans_in [B,6] f64 (source -> input, the closed form of get_affine_transform(c, s, 0, [in_w, in_h])),
    flip_width [B] i32)"""
    sizes, d = np.asarray(sizes, np.int64), np.asarray(draws, f64)
    h, w = sizes[:, 0], sizes[:, 1]
    in_h, in_w = (int(v) for v in input_hw)
    out_h, out_w = in_h // int(down_ratio), in_w // int(down_ratio)
    bad = (h < 1) | (w < 1)
    cx, cy = (w.astype(f64) / 2.0).astype(f32), (h.astype(f64) / 2.0).astype(f32)
    s = np.maximum(h, w).astype(f64)
    with np.errstate(all="ignore"):
        if rand_crop:
            s = s * d[:, 0]
            cx, cy = d[:, 1].astype(f32), d[:, 2].astype(f32)
        else:
            cf, sf = float(shift), float(scale)
            cx = (cx.astype(f64) + s * np.minimum(np.maximum(d[:, 0] * cf, -2.0 * cf), 2.0 * cf)).astype(f32)
            cy = (cy.astype(f64) + s * np.minimum(np.maximum(d[:, 1] * cf, -2.0 * cf), 2.0 * cf)).astype(f32)
            s = s * np.minimum(np.maximum(d[:, 2] * sf + 1.0, 1.0 - sf), 1.0 + sf)
        flipped = d[:, 3] < float(flip_prop)
        cx = np.where(flipped, (w.astype(f32) - cx) - f32(1.0), cx).astype(f32)
        s32 = s.astype(f32).astype(f64)
        dcx, dcy = cx.astype(f64), cy.astype(f64)
        zero = np.zeros_like(s32)
        k = out_w / s32
        trans_out = np.stack([k, zero, out_w * 0.5 - k * dcx, zero, k, out_h * 0.5 - k * dcy], 1)
        ki = in_w / s32
        trans_in = np.stack([ki, zero, in_w * 0.5 - ki * dcx, zero, ki, in_h * 0.5 - ki * dcy], 1)
        r = s32 / in_w
        ox, oy = dcx - r * (in_w * 0.5), dcy - r * (in_h * 0.5)
        mat_in = np.stack([np.where(flipped, -r, r), zero, np.where(flipped, (w - 1).astype(f64) - ox, ox), zero, r, oy], 1).astype(f32)
    flip_width = np.where(flipped, w, 0).astype(np.int32)
    mat_in[bad], trans_out[bad], trans_in[bad], flip_width[bad] = 0, 0, 0, 0
    return dict(c=np.stack([cx, cy], 1), s=s, flipped=flipped & ~bad, mat_in=mat_in, trans_out=trans_out, trans_in=trans_in,
                flip_width=flip_width)


def three_point_solve(src, dst):
    """the 2 x 3 float64 matrix that maps the three src points onto the three dst points (what the fixture's cv2 stub runs)"""
    a = np.concatenate([np.asarray(src, f64), np.ones((3, 1))], 1)
    return np.linalg.solve(a, np.asarray(dst, f64)).T.copy()


def solve_bound(c, s, dst_w):
    """[6] bound on |closed form - the reference's solve| per entry of the 2 x 3 matrix for c (fp32 pair), s (float64), dst_w"""
    cx, cy = abs(float(c[0])), abs(float(c[1]))
    s32 = float(f32(s))
    h = s32 / 2.0
    assert s32 > 0 and max(cx, cy) / s32 < 2.0 ** 12
    k = dst_w / s32
    rho_x, rho_y = U * (cx + cy + 3.0 * h) / h, U * (cy + h) / h
    a = np.array([[float(c[0]), float(c[1]), 1.0], [float(c[0]), float(c[1]) - h, 1.0], [float(c[0]) - h, float(c[1]) - h, 1.0]])
    big = max(k, k * cx + dst_w, k * cy + dst_w)
    lu = 9.0 * 2.0 ** -53 * np.linalg.cond(a, np.inf) * big
    return SLACK * np.array([k * rho_x, 0.0, k * rho_x * cx, 0.0, k * rho_y, k * rho_y * cy]) + lu


# ---------------------------------------------------------------------------------------------------- the sampler
def _fma32(a, b, c):
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def sample(img, hw, mat, out_hw):
    """img [Hs,Ws,3] u8, hw = the sample's own (h, w) (clamped to the array), mat [6] f32 -> [out_h,out_w,3] fp32 in grey levels"""
    Hs, Ws = img.shape[:2]
    h, w = min(max(int(hw[0]), 0), Hs), min(max(int(hw[1]), 0), Ws)
    m = np.asarray(mat, f32)
    if h == 0 or w == 0:
        return np.zeros((out_hw[0], out_hw[1], 3), f32)
    yy, xx = np.meshgrid(np.arange(out_hw[0]), np.arange(out_hw[1]), indexing="ij")
    x, y = xx.astype(f32), yy.astype(f32)
    with np.errstate(all="ignore"):
        sx = (_fma32(np.broadcast_to(m[0], x.shape), x, m[1] * y) + m[2]).astype(f32)
        sy = (_fma32(np.broadcast_to(m[4], y.shape), y, m[3] * x) + m[5]).astype(f32)
        ok = (sx > -1) & (sx < f32(w)) & (sy > -1) & (sy < f32(h))            # NaN fails every comparison
    sx, sy = np.where(ok, sx, f32(0)), np.where(ok, sy, f32(0))
    xf, yf = np.floor(sx), np.floor(sy)
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    lx, ly = (sx - xf).astype(f32), (sy - yf).astype(f32)
    v = np.zeros(x.shape + (3,), f32)
    for q in range(4):
        ty, tx = y0 + (q >> 1), x0 + (q & 1)
        wt = ((ly if q >> 1 else f32(1) - ly) * (lx if q & 1 else f32(1) - lx)).astype(f32)
        tap = ok & (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
        p = img[np.clip(ty, 0, Hs - 1), np.clip(tx, 0, Ws - 1)].astype(f32)
        v = np.where(tap[..., None], _fma32(np.broadcast_to(wt[..., None], v.shape), p, v), v)
    return v


def bf16_bits(x):
    """fp32 -> bf16 bit patterns (uint16), round to nearest even; NaN stays NaN"""
    b = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def plain(v, mean, std):
    """colour NULL: md_image_preprocess's fma(v, 1 / 255, -mean) / std on grey levels v [..., 3] -> fp32"""
    mean, std = np.asarray(mean, f32), np.asarray(std, f32)
    return (_fma32(v, np.broadcast_to(f32(1.0) / f32(255.0), v.shape), np.broadcast_to(-mean, v.shape)) / std).astype(f32)


# ---------------------------------------------------------------------------------------------------- the colour chain
def grey(x32):
    x = x32.astype(f64)
    return (GREY[0] * x[..., 0] + GREY[1] * x[..., 1]) + GREY[2] * x[..., 2]


def exact_mean(g):
    return math.fsum(g.ravel().tolist()) / g.size


def colour(x32, col, mean, std, gs_mean=None):
    """x32 [H,W,3] fp32 (the 0..1 image, BGR), col [8] f64 -> dict(x: the float64 chain, y: fp32 normalised, g, gs_mean); gs_mean None:
    the exactly rounded mean of the grey"""
    col = np.asarray(col, f64)
    g = grey(x32)
    m = exact_mean(g) if gs_mean is None else float(gs_mean)
    x = x32.astype(f64)
    od = col[6]
    order = ORDERS[int(od)] if 0.0 <= od <= 5.0 else ()
    for f in order:
        if f == 0:
            x = x * col[0]
        elif f == 1:
            x = col[1] * x + (1.0 - col[1]) * m
        else:
            x = col[2] * x + (1.0 - col[2]) * g[..., None]
    x = x + col[3:6]
    mean, std = np.asarray(mean, f32), np.asarray(std, f32)
    y = ((x.astype(f32) - mean) / std).astype(f32)
    return dict(x=x, y=y, g=g, gs_mean=m)


def colour_bound(x32, col, mean, std):
    """[H,W,3] bound on |the reference's inp - colour()'s y| for the reference's fp32 sequence (module docstring)"""
    col = np.asarray(col, f64)
    g = grey(x32)
    n = g.size
    m = exact_mean(g)
    e_g = 4.0 * U * g[..., None]
    e_m = (30.0 + max(0, math.ceil(math.log2(max(n, 1) / 128.0)))) * U * m
    x = x32.astype(f64)
    e = np.zeros_like(x)
    for f in ORDERS[int(col[6])]:
        a = col[f]
        if f == 0:
            x = x * a
            e = abs(a) * e + 2.0 * U * np.abs(x)
        else:
            x2, e2 = (m, e_m) if f == 1 else (g[..., None], e_g)
            ax, bx = a * x, (1.0 - a) * x2
            x = ax + bx
            e = abs(a) * e + 2.0 * U * np.abs(ax) + abs(1.0 - a) * e2 + 2.0 * U * np.abs(bx) + U * np.abs(x)
    x = x + col[3:6]
    e = e + U * np.abs(x)
    mean, std = np.asarray(mean, f64), np.asarray(std, f64)
    y = (x - mean) / std
    ref = (e + U * np.abs(x - mean)) / std + U * np.abs(y)
    own = (U * np.abs(x) + U * np.abs(x - mean)) / std + U * np.abs(y)
    return SLACK * (ref + own)


def image(img, sizes, mat_in, mean, std, out_hw, col=None, pad=(0, 0), C=8):
    """md_cn_aug_image: img [B,Hs,Ws,3] u8, sizes [B,2], mat_in [B,6] f32, col [B,8] f64 or None -> the bf16 bit patterns
    [B, pad_lo + out_h + pad_hi, pad_lo + out_w + pad_hi, C] (uint16)"""
    B = img.shape[0]
    ho, wo = out_hw
    lo, hi = pad
    out = np.zeros((B, ho + lo + hi, wo + lo + hi, C), np.uint16)
    for b in range(B):
        v = sample(img[b], sizes[b], mat_in[b], out_hw)
        if col is None:
            y = plain(v, mean, std)
        else:
            x32 = (v * (f32(1.0) / f32(255.0))).astype(f32)
            y = colour(x32, col[b], mean, std)["y"]
        out[b, lo:lo + ho, lo:lo + wo, :3] = bf16_bits(y)
    return out


def reversed_sum(g):
    """the float64 sum of g taken from the last element to the first (the mean sensitivity check)"""
    acc = 0.0
    for t in g.ravel()[::-1].tolist():
        acc += t
    return acc


def bf16_differences(got, want):
    """(elements that differ, the largest difference in bf16 ulps: the distance of the bit patterns as sign-magnitude integers)"""
    def key(b):
        b = b.astype(np.int64)
        return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)
    d = np.abs(key(np.asarray(got)) - key(np.asarray(want)))
    return int((d != 0).sum()), int(d.max()) if d.size else 0
