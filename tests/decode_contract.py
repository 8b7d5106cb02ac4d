"""The decode kernels' contract (include/minddet_hip.h) in float64 torch: md_rpn_decode, md_rcnn_scores, md_rcnn_decode_selected,
md_mask_select, md_yolo_decode, md_yolov8_decode, md_heat_peaks, md_centernet_assemble and md_centerpoint_decode -- a reference of
every output, an elementwise bound on how far the kernel's fp32 value may lie from it, and the data generators of
tests/test_decode_production_gpu.py.  Shared with tests/test_decode_reference_cpu.py (the references against the numpy oracles, the
generators' plants, the either-outcome cap).  Pattern: tests/conv_contract.py.

Error model (u = 2^-24, the unit roundoff of fp32 round to nearest; the build has no fast-math flags):

* A value is carried as T(v, e): v the float64 value of the operation sequence applied to the exact inputs, e a bound on
  |kernel's fp32 value - v|.  Inputs (bf16 head values, fp32 tensors and attribute constants) are exact: e = 0.
* Each plain fp32 operation (+, -, *, /: the division is the correctly rounded v_div_scale / v_div_fmas / v_div_fixup sequence) rounds
  once: |fl(y) - y| <= u |y|.  The propagation of the operands' errors is written out exactly (|a| e_b + |b| e_a + e_a e_b for a
  product, (e_a + |a / b| e_b) / (|b| - e_b) for a quotient), and each rounding is charged 2 u |y| -- the factor 2 margin of the conv
  suite for the ulp-versus-relative slack.  A contraction of a * b + c into one fma rounds once instead of twice and stays inside.
* expf(x) compiles to an extended-precision range reduction (x log2 e as a head + tail pair, n = rint(head)), v_exp_f32 of the reduced
  argument (1 ulp = 2 u relative) and v_ldexp_f32 (exact): relative error <= 2 u + u = 3 u (the reduced argument's own rounding is below
  u / 2, times ln 2); with the margin EXPF = 6 u.  The input's error e_x adds exp(v) (exp(e_x) - 1).
* sigmoid of an exact bf16 x, 1.0f / (1.0f + expf(-x)): E = expf(-x) errs by <= 3 u relative, 1 + E by u, the quotient by u; the
  derivative of 1 / (1 + E) with respect to E damps E's error by E / (1 + E) <= 1, so the relative error of the result is <= 5 u, and
  SIG = 10 u with the margin.  Where the result leaves the normal range the relative term does not hold: for x < -88.72 expf(-x)
  overflows to +inf and the kernel returns 0, and just above that the quotient is subnormal (or flushed to zero); |exact| < 2^-126
  there, so an absolute floor of TINY = 2^-126 is added to every sigmoid bound rather than a wider relative term.
* fminf / fmaxf clamps are 1-Lipschitz; where the whole interval v +- e lies past a clip value the kernel returns that value exactly
  (e = 0).
* A sum of n terms in an unspecified order (a wave's butterfly, a sequential loop) errs by <= gamma_{n-1} sum(|t| + e_t) + sum e_t
  (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4) with the margin unit 2 u.
* atan2f: the OpenCL accuracy requirement of 6 ulp (12 u relative), with the margin 24 u, plus the TINY floor.

Discrete outputs (labels, peak flags, threshold pass / fail, -FLT_MAX / -1 / 0 fills) must match exactly, except where the float64
inputs of the decision lie within the derived bound of its boundary: there either outcome is accepted, and each reference returns
how many of its decisions took that branch.  The tests assert that share is at most CAP."""
import math

import numpy as np
import torch

U = 2.0 ** -24
RND = 2 * U            # one fp32 rounding, with the margin
EXPF = 6 * U           # expf relative error, with the margin
SIG = 10 * U           # fp32 sigmoid relative error, with the margin
ATAN2 = 24 * U         # atan2f relative error (6 ulp), with the margin
TINY = 2.0 ** -126     # absolute floor where a sigmoid leaves the normal range
FLT_MAX = float(np.finfo(np.float32).max)
CAP = 1e-3             # the largest share of a case's decisions that may take the either-outcome branch
N_BF16_FINITE = 65280


def f32(x):
    """the float64 value of the fp32 number nearest x (an attribute constant as the kernel holds it)"""
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------------------------
# tracked values
# ---------------------------------------------------------------------------------------------------------------------------------
class T:
    """v: float64 value of the operation sequence on the exact inputs; e: bound on |kernel fp32 value - v|"""

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    def __getitem__(self, i):
        return T(self.v[i], self.e[i])


def _t(x, like):
    return x if isinstance(x, T) else T(torch.full_like(like, float(x)))


def _rnd(v, e):
    return T(v, e + RND * (v.abs() + e))


def add(a, b):
    a, b = _t(a, b.v if isinstance(b, T) else None), _t(b, a.v)
    return _rnd(a.v + b.v, a.e + b.e)


def sub(a, b):
    a, b = _t(a, b.v if isinstance(b, T) else None), _t(b, a.v)
    return _rnd(a.v - b.v, a.e + b.e)


def mul(a, b):
    a, b = _t(a, b.v if isinstance(b, T) else None), _t(b, a.v)
    return _rnd(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e)


def div(a, b):
    a, b = _t(a, b.v if isinstance(b, T) else None), _t(b, a.v)
    v = a.v / b.v
    assert bool((b.v.abs() > b.e).all()), "divisor interval contains zero"
    return _rnd(v, (a.e + v.abs() * b.e) / (b.v.abs() - b.e))


def neg(a):
    return T(-a.v, a.e)


def expf(a):
    v = torch.exp(a.v)
    e = v * torch.expm1(a.e)
    return T(v, e + EXPF * (v + e))


def sigmoid(x):
    """1.0f / (1.0f + expf(-x)) of exact values x (float64 of bf16)"""
    v = 1.0 / (1.0 + torch.exp(-x))
    return T(v, SIG * v + TINY)


def clamp(a, lo, hi):
    """fminf(fmaxf(a, lo), hi) with fp32 constants lo <= hi"""
    v = a.v.clamp(lo, hi)
    sure = (a.v - a.e >= hi) | (a.v + a.e <= lo)
    return T(v, torch.where(sure, torch.zeros_like(a.e), a.e))


def gamma(n_terms):
    m = max(n_terms - 1, 0)
    return m * RND / (1 - m * RND)


def fsum(a, dim):
    """sum over `dim` in an unspecified order"""
    n = a.v.shape[dim]
    return T(a.v.sum(dim), a.e.sum(dim) + gamma(n) * (a.v.abs() + a.e).sum(dim))


def atan2f(y, x):
    v = torch.atan2(y, x)
    return T(v, ATAN2 * v.abs() + TINY)


def stack(ts, dim=-1):
    return T(torch.stack([t.v for t in ts], dim), torch.stack([t.e for t in ts], dim))


def decision(a, thr):
    """a > thr for a tracked a: (surely true, surely false); neither = either outcome"""
    return a.v - a.e > thr, a.v + a.e <= thr


# ---------------------------------------------------------------------------------------------------------------------------------
# bf16 helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def all_finite_bf16(device="cpu"):
    """the 65280 finite bf16 numbers (both zeros included), as a bf16 tensor in bit-pattern order"""
    p = torch.arange(65536, dtype=torch.int32)
    p = p[((p >> 7) & 0xFF) != 0xFF]
    p = torch.where(p >= 32768, p - 65536, p).to(torch.int16)
    assert p.numel() == N_BF16_FINITE
    return p.view(torch.bfloat16).to(device)


def bf16_nan(shape, device):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device=device)


def d64(t):
    return t.double()


# ---------------------------------------------------------------------------------------------------------------------------------
# box decode (twostage.hip decode_box; md_delta2bbox_attrs)
# ---------------------------------------------------------------------------------------------------------------------------------
def decode_box(r, d, dec):
    """r [..., 4] fp32 box (x1, y1, x2, y2), d [..., 4] bf16 deltas (float64 of both) -> T [..., 4].  dec: the md_delta2bbox_attrs
    dict.  mean / std, dw / dh clamped to +-max_ratio, centre / size, exp, clip to [0, clip_w] x [0, clip_h] when both are > 0."""
    m = [f32(v) for v in dec["means"]]
    s = [f32(v) for v in dec["stds"]]
    mr = f32(dec["max_ratio"])
    dd = [add(mul(T(d[..., j]), s[j]), m[j]) for j in range(4)]
    dw, dh = clamp(dd[2], -mr, mr), clamp(dd[3], -mr, mr)
    x1, y1, x2, y2 = (T(r[..., j]) for j in range(4))
    px, py = mul(add(x1, x2), 0.5), mul(add(y1, y2), 0.5)
    pw, ph = sub(x2, x1), sub(y2, y1)
    gw, gh = mul(pw, expf(dw)), mul(ph, expf(dh))
    gx, gy = add(px, mul(pw, dd[0])), add(py, mul(ph, dd[1]))
    hw, hh = mul(gw, 0.5), mul(gh, 0.5)
    out = [sub(gx, hw), sub(gy, hh), add(gx, hw), add(gy, hh)]
    cw, ch = f32(dec["clip_w"]), f32(dec["clip_h"])
    if cw > 0 and ch > 0:
        out = [clamp(o, 0.0, cw if j % 2 == 0 else ch) for j, o in enumerate(out)]
    return stack(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# references.  Each returns (outputs, n_decisions, n_either): outputs maps an output name to an Expect.
# ---------------------------------------------------------------------------------------------------------------------------------
class Expect:
    """What one output (or a region of it) may hold, elementwise.
    val: T of the computed value (None: no value is allowed); fill: the exact fill (a float, or a float64 tensor of fp32
    values; None: no fill);
    want_val / want_fill: bool masks of where each form is allowed (both True = either outcome).
    For integer outputs val is None and `ok` is a callable got -> bool tensor."""

    def __init__(self, val=None, fill=None, want_val=None, want_fill=None, ok=None):
        self.val, self.fill, self.want_val, self.want_fill, self.ok = val, fill, want_val, want_fill, ok


def ints(want):
    return Expect(ok=lambda got: got == want)


def check(got, x):
    """got (a device or host tensor) against an Expect -> (n_bad, worst err / bound over the elements taken as values, first bad index)"""
    if x.ok is not None:
        bad = ~x.ok(got.long())
        worst = 0.0
    else:
        g = got.double()
        ok = torch.zeros(g.shape, dtype=torch.bool, device=g.device)
        is_fill = torch.zeros_like(ok)
        if x.fill is not None:
            fb = (x.fill.to(torch.float32).view(torch.int32) if torch.is_tensor(x.fill)
                  else torch.tensor([x.fill], dtype=torch.float32).view(torch.int32).item())
            is_fill = got.contiguous().view(torch.int32) == fb
            ok |= x.want_fill & is_fill
        worst = 0.0
        if x.val is not None:
            err = (g - x.val.v).abs()
            within = torch.isfinite(g) & (err <= x.val.e)
            ok |= x.want_val & within
            as_val = x.want_val & ~(is_fill & x.want_fill)
            if bool(as_val.any()):
                r = torch.where(err == 0, torch.zeros_like(err), err / x.val.e)[as_val]
                r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
                worst = float(r.max())
        bad = ~ok
    nb = int(bad.sum())
    first = tuple(int(v) for v in bad.nonzero()[0]) if nb else None
    return nb, worst, first


def yolo(head, a):
    """md_yolo_decode over the rows it writes: head [b, H, W, Cp] -> outputs over [b, H*W*A] (row = loc * A + anchor)"""
    b, H, W, _ = head.shape
    nc, A = a["num_classes"], a["num_anchors"]
    per = 5 + nc
    x = d64(head[..., :A * per]).reshape(b, H * W * A, per)
    row = torch.arange(H * W * A, device=head.device)
    loc, an = row // A, row % A
    gx, gy = d64(loc % W), d64(loc // W)
    aw = torch.tensor([f32(a["anchors"][2 * i]) for i in range(A)], dtype=torch.float64, device=head.device)[an]
    ah = torch.tensor([f32(a["anchors"][2 * i + 1]) for i in range(A)], dtype=torch.float64, device=head.device)[an]
    stride = f32(a["stride"])
    s = [sigmoid(x[..., j]) for j in range(5)]
    cx = mul(add(sub(mul(s[0], 2.0), 0.5), T(gx.expand_as(x[..., 0]))), stride)
    cy = mul(add(sub(mul(s[1], 2.0), 0.5), T(gy.expand_as(x[..., 0]))), stride)
    w2, h2 = mul(s[2], 2.0), mul(s[3], 2.0)
    w = mul(mul(w2, w2), T(aw.expand_as(x[..., 0])))
    hh = mul(mul(h2, h2), T(ah.expand_as(x[..., 0])))
    hw_, hh_ = mul(w, 0.5), mul(hh, 0.5)
    boxes = stack([sub(cx, hw_), sub(cy, hh_), add(cx, hw_), add(cy, hh_)])
    best, lab = x[..., 5:].max(-1)           # first index on ties
    conf = mul(s[4], sigmoid(best))
    thr = f32(a["conf_thres"])
    op, of = decision(s[4], thr)
    cp, cf = decision(conf, thr)
    sp, sf = op & cp, of | cf
    either = ~(sp | sf)
    out = dict(boxes=Expect(val=boxes, want_val=torch.ones(boxes.v.shape, dtype=torch.bool, device=head.device),
                            want_fill=torch.zeros(boxes.v.shape, dtype=torch.bool, device=head.device)),
               scores=Expect(val=conf, fill=-FLT_MAX, want_val=~sf, want_fill=~sp),
               labels=ints(lab))
    return out, sp.numel(), int(either.sum())


def yolov8(head, a):
    """md_yolov8_decode over the rows it writes: head [b, H, W, Cp] -> outputs over [b, H*W]"""
    b, H, W, _ = head.shape
    nc, R = a["num_classes"], a["reg_max"]
    x = d64(head[..., :4 * R + nc]).reshape(b, H * W, 4 * R + nc)
    bins = x[..., :4 * R].reshape(b, H * W, 4, R)
    mx = bins.max(-1, keepdim=True).values
    t = sub(T(bins), T(mx.expand_as(bins)))
    p = expf(t)
    den = fsum(p, -1)
    idx = torch.arange(R, dtype=torch.float64, device=head.device)
    num = fsum(mul(p, T(idx.expand_as(p.v))), -1)
    d = div(num, den)                                     # [b, HW, 4]
    loc = torch.arange(H * W, device=head.device)
    ax = T((d64(loc % W) + 0.5).expand_as(d.v[..., 0]))
    ay = T((d64(loc // W) + 0.5).expand_as(d.v[..., 0]))
    s = f32(a["stride"])
    boxes = stack([mul(sub(ax, d[..., 0]), s), mul(sub(ay, d[..., 1]), s), mul(add(ax, d[..., 2]), s), mul(add(ay, d[..., 3]), s)])
    best, lab = x[..., 4 * R:].max(-1)
    conf = sigmoid(best)
    sp, sf = decision(conf, f32(a["conf_thres"]))
    ones = torch.ones(boxes.v.shape, dtype=torch.bool, device=head.device)
    out = dict(boxes=Expect(val=boxes, want_val=ones, want_fill=~ones),
               scores=Expect(val=conf, fill=-FLT_MAX, want_val=~sf, want_fill=~sp),
               labels=ints(lab))
    return out, sp.numel(), int((~(sp | sf)).sum())


def rpn_decode(head, anchors, idx, cnt, a):
    """md_rpn_decode: head [b, H, W, Cp], anchors [HWA, 4], idx [b, k], cnt [b] -> boxes [b, k, 4], scores [b, k]"""
    b, H, W, Cp = head.shape
    A = a["num_anchors"]
    k = idx.shape[1]
    live = torch.arange(k, device=head.device)[None] < cnt[:, None].long()
    ii = torch.where(live, idx.long(), torch.zeros_like(idx.long()))
    h = d64(head).reshape(b, H * W, Cp)
    loc, an = ii // A, ii % A
    rows = torch.gather(h, 1, loc[..., None].expand(b, k, Cp))     # [b, k, Cp]
    logit = torch.gather(rows, 2, an[..., None])[..., 0]
    dl = torch.stack([torch.gather(rows, 2, (A + an * 4 + j)[..., None])[..., 0] for j in range(4)], -1)
    boxes = decode_box(d64(anchors)[ii], dl, a["decode"])
    boxes = T(torch.where(live[..., None], boxes.v, torch.zeros_like(boxes.v)), torch.where(live[..., None], boxes.e, torch.zeros_like(boxes.e)))
    sc = sigmoid(logit)
    l4 = live[..., None].expand_as(boxes.v)
    return dict(boxes=Expect(val=boxes, fill=0.0, want_val=l4, want_fill=~l4),
                scores=Expect(val=sc, fill=-FLT_MAX, want_val=live, want_fill=~live)), live.numel(), 0


def rcnn_scores(cls_reg, roi_cnt, a, rows=None):
    """md_rcnn_scores: cls_reg [R, Cp] (rows of images [i0, i1) when `rows` = (i0, i1, post)) -> cand [R, nc] (the [B, post * nc]
    output viewed per RoI).  softmax over the nc + 1 logits (background last), p > score_thr on valid slots, else -FLT_MAX."""
    nc = a["num_classes"]
    x = d64(cls_reg[:, :nc + 1])
    post = rows[2]
    j = torch.arange(x.shape[0], device=x.device)
    img = rows[0] + j // post
    valid = (j % post) < roi_cnt.long()[img]
    m = x.max(-1, keepdim=True).values
    ex = expf(sub(T(x), T(m.expand_as(x))))
    ssum = fsum(ex, -1)
    p = div(ex[:, :nc], T(ssum.v[:, None].expand(-1, nc), ssum.e[:, None].expand(-1, nc)))
    sp, sf = decision(p, f32(a["score_thr"]))
    v = valid[:, None].expand_as(p.v)
    sp, sf = sp & v, sf | ~v
    return dict(cand=Expect(val=p, fill=-FLT_MAX, want_val=~sf, want_fill=~sp)), int(v.sum()), int((~(sp | sf)).sum())


def rcnn_decode_selected(cls_reg, rois, sel_idx, sel_cnt, a, post):
    """md_rcnn_decode_selected for the images of sel_idx [b, npre] (cls_reg / rois: those images' rows) -> boxes, labels"""
    nc, reg0 = a["num_classes"], a["reg_offset"]
    b, npre = sel_idx.shape
    live = torch.arange(npre, device=sel_idx.device)[None] < sel_cnt.long()[:, None]
    ii = torch.where(live, sel_idx.long(), torch.zeros_like(sel_idx.long()))
    j, c = ii // nc, ii % nc
    r = torch.arange(b, device=ii.device)[:, None] * post + j
    ch = reg0 + c * 4
    x = d64(cls_reg)
    d = torch.stack([x[r, ch + t] for t in range(4)], -1)
    boxes = decode_box(d64(rois)[r][..., 1:], d, a["decode"])
    boxes = T(torch.where(live[..., None], boxes.v, torch.zeros_like(boxes.v)), torch.where(live[..., None], boxes.e, torch.zeros_like(boxes.e)))
    l4 = live[..., None].expand_as(boxes.v)
    lab = torch.where(live, c, torch.full_like(c, -1))
    return dict(boxes=Expect(val=boxes, fill=0.0, want_val=l4, want_fill=~l4), labels=ints(lab)), live.numel(), 0


def mask_select(logits, dets, nc):
    """md_mask_select: logits [r, S, S, Cpad], dets [r, 6] -> masks [r, S, S]: sigmoid of the detection's own class channel, 0 for score
    <= 0 or a label outside [0, nc)"""
    r, S = logits.shape[0], logits.shape[1]
    score, label = dets[:, 4], dets[:, 5].long()
    valid = (score > 0) & (label >= 0) & (label < nc)
    lab = torch.where(valid, label, torch.zeros_like(label))
    x = torch.gather(d64(logits), 3, lab.view(r, 1, 1, 1).expand(r, S, S, 1))[..., 0]
    v = valid.view(r, 1, 1).expand(r, S, S)
    sg = sigmoid(x)
    z = torch.zeros_like(sg.v)
    return dict(masks=Expect(val=T(torch.where(v, sg.v, z), torch.where(v, sg.e, z)), fill=0.0, want_val=v, want_fill=~v)), v.numel(), 0


NEIGHBOURS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]


def heat_peaks(head, a):
    """md_heat_peaks: head [b, H, W, Cp] -> (hm T [b, nc, H, W] = clip(sigmoid, fp32 lo, fp32 hi), heat Expect, peak flags,
    n_decisions, n_either).  A cell is a peak when its value is >= every in-image 3 x 3 neighbour's; out-of-image cells are ignored.  A
    neighbour decides the flag for sure unless its float64 value lies within the two bounds of the centre's while the bf16 logits
    differ (equal logits give equal fp32 values: a tie, so a peak either way); exact (clipped) values compare exactly."""
    c0, nc = a["c0"], a["num_classes"]
    x = d64(head[..., c0:c0 + nc]).permute(0, 3, 1, 2)          # [b, nc, H, W]
    hm = clamp(sigmoid(x), f32(a["lo"]), f32(a["hi"]))
    b, _, H, W = x.shape
    pad = lambda t, val: torch.nn.functional.pad(t, (1, 1, 1, 1), value=val)
    pv, pe, px = pad(hm.v, -math.inf), pad(hm.e, 0.0), pad(x, math.nan)
    sure_not = torch.zeros(x.shape, dtype=torch.bool, device=x.device)
    amb = torch.zeros_like(sure_not)
    for dy, dx in NEIGHBOURS:
        nv, ne, nx = (t[:, :, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for t in (pv, pe, px))
        band = ((nv - hm.v).abs() <= ne + hm.e) & (ne + hm.e > 0) & (nx != x) & torch.isfinite(nv)
        amb |= band
        sure_not |= (nv > hm.v) & ~band
    peak = ~sure_not & ~amb                     # surely a peak
    either = amb & ~sure_not
    heat = Expect(val=hm, fill=0.0, want_val=peak | either, want_fill=sure_not | either)
    return hm, heat, peak, peak.numel(), int(either.sum())


def centernet_assemble(top_score, top_ind2, cls_inds, wh, reg):
    """md_centernet_assemble as the header writes it: j = top_ind2, cls = j / K, ind = cls_inds[b, j], (xs, ys) = (ind % W, ind / W)
    + reg (+ 0.5 without reg), det = (xs - w / 2, ys - h / 2, xs + w / 2, ys + h / 2, score, cls)"""
    b, K = top_score.shape
    H, W = wh.shape[2], wh.shape[3]
    j = top_ind2.long()
    cls = j // K
    ind = torch.gather(cls_inds.reshape(b, -1).long(), 1, j)
    whf, w_, h_ = wh.reshape(b, 2, H * W), None, None
    w_ = T(torch.gather(d64(whf[:, 0]), 1, ind))
    h_ = T(torch.gather(d64(whf[:, 1]), 1, ind))
    if reg is not None:
        rf = reg.reshape(b, 2, H * W)
        xs = add(T(d64(ind % W)), T(torch.gather(d64(rf[:, 0]), 1, ind)))
        ys = add(T(d64(ind // W)), T(torch.gather(d64(rf[:, 1]), 1, ind)))
    else:
        xs, ys = add(T(d64(ind % W)), 0.5), add(T(d64(ind // W)), 0.5)
    hw, hh = div(w_, 2.0), div(h_, 2.0)
    det = stack([sub(xs, hw), sub(ys, hh), add(xs, hw), add(ys, hh), T(d64(top_score)), T(d64(cls))])
    ones = torch.ones(det.v.shape, dtype=torch.bool, device=det.v.device)
    return dict(det=Expect(val=det, want_val=ones, want_fill=~ones), inds=ints(ind), cls=ints(cls)), 0, 0


NEG_HALF_PI = f32(-1.5707963267948966)


def centerpoint(head, a, y0=0):
    """md_centerpoint_decode: head [b, H, W, C] -> scores [b, HW], labels [b, HW], boxes [b, HW, 9], nms_boxes [b, HW, 7]"""
    b, H, W, C = head.shape
    ncls = a["num_classes"]
    f = d64(head).reshape(b, H * W, C)
    hml = f[..., a["off_hm"]:a["off_hm"] + ncls]
    sg = sigmoid(hml)
    best_logit, lab0 = hml.max(-1)                    # first arg-max of the logits
    sbest = sigmoid(best_logit)
    # a lower index may win where fp32 saturation ties the sigmoids: float64 sigma within twice the bound of the maximum's
    lower = (torch.arange(ncls, device=f.device)[None, None] < lab0[..., None]) & ((sbest.v[..., None] - sg.v) <= 2 * (sbest.e[..., None]))
    loc = torch.arange(H * W, device=f.device)
    gx, gy = d64(loc % W).expand(b, -1), d64(loc // W).expand(b, -1)
    osf = f32(a["out_size_factor"])
    xs = add(mul(mul(add(T(gx), T(f[..., a["off_reg"]])), osf), f32(a["voxel_size"][0])), f32(a["pc_range"][0]))
    ys = add(mul(mul(add(T(gy), T(f[..., a["off_reg"] + 1])), osf), f32(a["voxel_size"][1])), f32(a["pc_range"][1]))
    zs = T(f[..., a["off_height"]])
    dims = [expf(T(f[..., a["off_dim"] + j])) for j in range(3)]
    rot = atan2f(f[..., a["off_rot"]], f[..., a["off_rot"] + 1])
    if a["off_vel"] >= 0:
        vel = [T(f[..., a["off_vel"]]), T(f[..., a["off_vel"] + 1])]
    else:
        vel = [T(torch.zeros_like(gx)), T(torch.zeros_like(gx))]
    r = [f32(v) for v in a["post_center_range"]]
    s_in, s_out = torch.ones_like(gx, dtype=torch.bool), torch.zeros_like(gx, dtype=torch.bool)
    n_range_either = torch.zeros_like(s_in)
    for t, lo, hi in ((xs, r[0], r[3]), (ys, r[1], r[4]), (zs, r[2], r[5])):
        lo_in, lo_out = t.v - t.e >= lo, t.v + t.e < lo           # t >= lo surely / surely not
        hi_in, hi_out = t.v + t.e <= hi, t.v - t.e > hi           # t <= hi surely / surely not
        s_in &= lo_in & hi_in
        s_out |= lo_out | hi_out
    sp, sf = decision(sbest, f32(a["score_threshold"]))
    ok, masked = sp & s_in, sf | s_out
    either = ~(ok | masked)
    boxes = stack([xs, ys, zs, dims[0], dims[1], dims[2], vel[0], vel[1], rot])
    r2 = sub(neg(rot), -NEG_HALF_PI)
    nms = stack([xs, ys, zs, dims[1], dims[0], dims[2], r2])
    fill_nms = torch.zeros((b, H * W, 7), dtype=torch.float64, device=f.device)
    fill_nms[..., 6] = NEG_HALF_PI
    wv, wf = ~masked, ~ok

    def rows(x, n):
        return Expect(val=x, fill=None, want_val=wv[..., None].expand(-1, -1, n), want_fill=wf[..., None].expand(-1, -1, n))

    eb, en = rows(boxes, 9), rows(nms, 7)
    eb.fill, en.fill = 0.0, fill_nms

    def lab_ok(got):
        g = got
        first = g == lab0
        low = torch.zeros_like(first)
        for c in range(ncls):
            low |= (g == c) & lower[..., c]
        return torch.where(wf & wv, first | low | (g == -1), torch.where(wv, first | low, g == -1))

    return dict(scores=Expect(val=sbest, fill=-1.0, want_val=wv, want_fill=wf), labels=Expect(ok=lab_ok), boxes=eb, nms_boxes=en,
                lower=lower), ok.numel(), int(either.sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# data generators: Gaussian bf16 heads at a scale that balances each threshold decision, plus planted rows.  Each returns the op's
# inputs (in the op's parameter order) and a dict of what it planted, which tests/test_decode_reference_cpu.py verifies.
# ---------------------------------------------------------------------------------------------------------------------------------
TIE, SAT, LOW = 7, 11, 13      # planted class rows: r % PLANT_MOD
PLANT_MOD = 509


def logit(p):
    return math.log(p / (1.0 - p))


def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def _randn(shape, g, device, mean=0.0, std=1.0):
    return torch.randn(shape, generator=g, device=device) * std + mean


def _randint(lo, hi, shape, g, device):
    return torch.randint(lo, hi, shape, generator=g, device=device)


def _spread_all_bf16(flat, g, device):
    """write every finite bf16 value into randomly chosen elements of the 1-D bf16 view `flat` (when it has that many) -> positions"""
    if flat.numel() < N_BF16_FINITE:
        return None
    pos = torch.randperm(flat.numel(), generator=g, device=device)[:N_BF16_FINITE]
    flat[pos] = all_finite_bf16(device)
    return pos


def _plant_classes(cls, g, device, tie_value=4.0):
    """cls [rows, nc] float32 class logits.  rows r % PLANT_MOD == TIE: two indices i < j tie at the maximum (tie_value, the rest below
    it) -> label i;  SAT: logits 16 at i and 17 at j > i (both sigmoids round to 1.0 - 2^-24 or 1.0 in fp32) -> label j;  LOW: every logit
    below -87 (-100 ... -120), -90 at j >= 1 -> label j.  Returns {kind: (rows, expected label)}."""
    n, nc = cls.shape
    r = torch.arange(n, device=device)
    out = {}
    for kind in (TIE, SAT, LOW):
        rows = r[r % PLANT_MOD == kind]
        m = rows.numel()
        if m == 0 or nc < 2:
            continue
        i = _randint(0, nc - 1, (m,), g, device)
        j = i + 1 + (torch.rand((m,), generator=g, device=device) * (nc - 1 - i).float()).long()
        if kind == TIE:
            cls[rows] = cls[rows].clamp(max=tie_value - 1.0)
            cls[rows, i] = tie_value
            cls[rows, j] = tie_value
            out["tie"] = (rows, i)
        elif kind == SAT:
            cls[rows] = cls[rows].clamp(max=8.0)
            cls[rows, i] = 16.0
            cls[rows, j] = 17.0
            out["sat"] = (rows, j)
        else:
            j = 1 + _randint(0, nc - 1, (m,), g, device)
            cls[rows] = -100.0 - 20.0 * torch.rand((m, nc), generator=g, device=device)
            cls[rows, j] = -90.0
            out["low"] = (rows, j)
    return out


def gen_yolo(shape, a, seed, device):
    """head [B, H, W, Cp]: obj ~ N(logit(conf_thres), 2^2), the rest ~ N(0, 2^2); every finite bf16 value as an obj logit (levels with
    at least 65280 rows); planted class rows (_plant_classes); NaN in the Cp padding"""
    B, H, W, Cp = shape
    nc, A = a["num_classes"], a["num_anchors"]
    per = 5 + nc
    g = _gen(seed, device)
    x = _randn((B * H * W * A, per), g, device, std=2.0)
    x[:, 4] += logit(f32(a["conf_thres"]))
    plants = _plant_classes(x[:, 5:], g, device)
    head = bf16_nan((B, H, W, Cp), device)
    rows = x.to(torch.bfloat16)
    obj = rows[:, 4].clone()
    plants["obj"] = _spread_all_bf16(obj, g, device)
    rows[:, 4] = obj
    head[..., :A * per] = rows.view(B, H, W, A * per)
    return [head], plants


def gen_yolov8(shape, a, seed, device):
    """head [B, H, W, Cp]: DFL bins ~ N(0, 2^2); class logits ~ N(logit(conf_thres) - 4.8, 2^2) (the maximum of 80 sits near the
    threshold); planted class rows; NaN in the Cp padding"""
    B, H, W, Cp = shape
    nc, R = a["num_classes"], a["reg_max"]
    g = _gen(seed, device)
    x = _randn((B * H * W, 4 * R + nc), g, device, std=2.0)
    x[:, 4 * R:] += logit(f32(a["conf_thres"])) - 4.8
    plants = _plant_classes(x[:, 4 * R:], g, device)
    head = bf16_nan((B, H, W, Cp), device)
    head[..., :4 * R + nc] = x.to(torch.bfloat16).view(B, H, W, -1)
    return [head], plants


def _counts(B, k):
    """per image: 0, a third, all k, k - 1 (cycling)"""
    return torch.tensor([(0, k // 3, k, k - 1)[b % 4] for b in range(B)], dtype=torch.int32)


def _distinct_with_ends(B, n, k, g, device):
    """[B, k] int32: per image min(k, n) distinct indices of [0, n) in the first slots, the first (0) and the last (n - 1) among them
    at random positions; slots past n (k > n: a level with fewer anchors than the top-k's k) hold arbitrary valid indices"""
    m = min(k, n)
    out = _randint(0, n, (B, k), g, device).to(torch.int32)
    for b in range(B):
        p = torch.randperm(n - 2, generator=g, device=device)[:m - 2] + 1
        p = torch.cat([torch.tensor([0, n - 1], device=device), p])
        out[b, :m] = p[torch.randperm(m, generator=g, device=device)].to(torch.int32)
    return out


def _boxes(n, g, device, w, h, lo=4.0, hi=800.0, clip=False):
    """n fp32 boxes: centres uniform over [-0.1, 1.1] x the image, sizes log-uniform in [lo, hi]; clip: inside the image, >= 1 wide"""
    c = torch.rand((n, 2), generator=g, device=device) * 1.2 - 0.1
    c = c * torch.tensor([w, h], device=device)
    s = torch.exp(math.log(lo) + torch.rand((n, 2), generator=g, device=device) * math.log(hi / lo))
    b = torch.cat([c - s / 2, c + s / 2], 1)
    if clip:
        b[:, 0::2] = b[:, 0::2].clamp(0, w - 1)
        b[:, 1::2] = b[:, 1::2].clamp(0, h - 1)
        b[:, 2:] = torch.maximum(b[:, 2:], b[:, :2] + 1)
    return b.float().contiguous()


BIG_DELTA = 97     # planted deltas: r % BIG_DELTA == 3 -> (dw, dh) = (+big, -big), == 5 -> (-big, +big)


def gen_rpn(shapes, a, seed, device):
    """head [B, H, W, Cp] (objectness ~ N(0, 2^2), deltas ~ N(0, 1), NaN in the Cp padding), anchors [HWA, 4] (boxes that cross every
    image edge), idx [B, k] (distinct; the first and the last anchor in every image), cnt [B] (0, partial, k; at most the level's
    anchor count).  The selected logits run
    through the finite bf16 values from a per-call offset (all of them when B k >= 65280).  Planted: selected rows with |dw|, |dh| = 8
    past max_ratio."""
    (B, H, W, Cp), _, (_, k) = shapes[0], shapes[1], shapes[2]
    A = a["num_anchors"]
    g = _gen(seed, device)
    n = H * W * A
    head = bf16_nan((B, H, W, Cp), device)
    head[..., :5 * A] = _randn((B, H, W, 5 * A), g, device).to(torch.bfloat16)
    head[..., :A] = (head[..., :A].float() * 2).to(torch.bfloat16)
    cw, ch = a["decode"]["clip_w"], a["decode"]["clip_h"]
    anchors = _boxes(n, g, device, cw if cw > 0 else 1344.0, ch if ch > 0 else 800.0)
    idx = _distinct_with_ends(B, n, k, g, device)
    cnt = _counts(B, min(k, n)).to(device)
    live = torch.arange(k, device=device)[None] < cnt[:, None]
    bi, ji = live.nonzero(as_tuple=True)
    ids = idx[bi, ji].long()
    hf = head.view(B, H * W, Cp)
    allv = all_finite_bf16(device)
    off = int(_randint(0, N_BF16_FINITE, (1,), g, device))
    hf[bi, ids // A, ids % A] = allv[(off + torch.arange(bi.numel(), device=device)) % N_BF16_FINITE]
    big = []
    for m, sgn in ((3, 1.0), (5, -1.0)):
        s = (ji % BIG_DELTA) == m
        hf[bi[s], ids[s] // A, A + (ids[s] % A) * 4 + 2] = sgn * 8.0
        hf[bi[s], ids[s] // A, A + (ids[s] % A) * 4 + 3] = -sgn * 8.0
        big.append((bi[s], ji[s]))
    return [head, anchors, idx, cnt], dict(big=big, n_logits=bi.numel(), offset=off)


def gen_rcnn_scores(shapes, a, seed, device):
    """cls_reg [R, Cp]: the nc + 1 logits ~ N(0, 2^2), NaN in every other channel (deltas, padding); roi_cnt [B] (0, partial, post)"""
    (R, Cp), (B,) = shapes[0], shapes[1]
    nc = a["num_classes"]
    g = _gen(seed, device)
    x = bf16_nan((R, Cp), device)
    x[:, :nc + 1] = _randn((R, nc + 1), g, device, std=2.0).to(torch.bfloat16)
    return [x, _counts(B, R // B).to(device)], {}


def gen_rcnn_decode(shapes, a, seed, device, img_hw=(800.0, 1344.0)):
    """cls_reg [R, Cp]: deltas ~ N(0, 1), NaN in the logits and the padding; rois [R, 5] (b, clipped boxes); sel_idx [B, npre]
    (distinct; the first and the last candidate of every image), sel_cnt [B] (0, partial, npre).  Planted: candidates j with
    j % BIG_DELTA in (3, 5) get dw, dh = +-30 (x std 0.2 = 6, past max_ratio)."""
    (R, Cp), _, (B, npre) = shapes[0], shapes[1], shapes[2]
    nc, reg0 = a["num_classes"], a["reg_offset"]
    post = R // B
    g = _gen(seed, device)
    x = bf16_nan((R, Cp), device)
    d = _randn((R, nc, 4), g, device)
    j = torch.arange(nc, device=device)
    for m, sgn in ((3, 30.0), (5, -30.0)):
        s = (j % BIG_DELTA) == m
        d[:, s, 2], d[:, s, 3] = sgn, -sgn
    x[:, reg0:reg0 + 4 * nc] = d.reshape(R, 4 * nc).to(torch.bfloat16)
    cw, ch = a["decode"]["clip_w"], a["decode"]["clip_h"]
    rois = torch.zeros((R, 5), dtype=torch.float32, device=device)
    rois[:, 0] = (torch.arange(R, device=device) // post).float()
    rois[:, 1:] = _boxes(R, g, device, cw if cw > 0 else img_hw[1], ch if ch > 0 else img_hw[0], clip=True)
    sel = _distinct_with_ends(B, post * nc, npre, g, device)
    return [x, rois, sel, _counts(B, min(npre, post * nc)).to(device)], {}


MASK_PLANTS = {1: "score 0", 3: "negative score", 5: "label -1", 7: "label nc"}   # r % 10


def gen_mask(shapes, nc, seed, device):
    """logits [R, S, S, Cpad]: NaN except the label channel of the valid detections (~ N(0, 4^2), every finite bf16 value among them),
    dets [R, 6] (boxes, score in (0.05, 1], label in [0, nc)); rows r % 10 == 1, 3, 5, 7 carry score 0, a negative score, label -1 and
    label nc (MASK_PLANTS)"""
    (R, S, _, C), _ = shapes[0], shapes[1]
    g = _gen(seed, device)
    dets = torch.zeros((R, 6), dtype=torch.float32, device=device)
    dets[:, :4] = _boxes(R, g, device, 1344.0, 800.0, clip=True)
    dets[:, 4] = 0.05 + 0.95 * torch.rand((R,), generator=g, device=device)
    dets[:, 5] = _randint(0, nc, (R,), g, device).float()
    r = torch.arange(R, device=device)
    dets[r % 10 == 1, 4] = 0.0
    dets[r % 10 == 3, 4] = -0.5
    dets[r % 10 == 5, 5] = -1.0
    dets[r % 10 == 7, 5] = float(nc)
    valid = (dets[:, 4] > 0) & (dets[:, 5] >= 0) & (dets[:, 5] < nc)
    logits = bf16_nan((R, S, S, C), device)
    vr = valid.nonzero()[:, 0]
    vals = _randn((vr.numel(), S * S), g, device, std=4.0).to(torch.bfloat16).reshape(-1)
    pos = _spread_all_bf16(vals, g, device)
    logits.view(R, S * S, C)[vr[:, None], torch.arange(S * S, device=device)[None], dets[vr, 5].long()[:, None]] = vals.view(-1, S * S)
    return [logits, dets], dict(valid=valid, all_bf16=pos is not None)


def heat_plateaus(H, W):
    """(name, cells [(y, x)], ring value, block value(s)) planted into every image of a heat map, each in its own class channel: equal-
    logit and clipped (different logits, one clipped value) blocks straddling the 8 x 64 tile seams and touching the image border, and a
    block with a higher neighbour across a seam"""
    out = []
    if H >= 18 and W >= 70:
        out.append(("seam", [(7, 63), (7, 64), (8, 63), (8, 64)], 0.0, [6.0] * 4, [True] * 4))
        out.append(("seam_clip_hi", [(15, 63), (15, 64), (16, 63), (16, 64)], 0.0, [10.0, 12.0, 11.0, 14.0], [True] * 4))
        out.append(("seam_clip_lo", [(y, x) for y in (22, 23, 24, 25) for x in (62, 63, 64, 65)], -20.0,
                    [-12.0 - 0.5 * i for i in range(16)], [True] * 16))
    if H >= 34 and W >= 70:
        out.append(("seam_higher", [(31, 63), (31, 64), (32, 63), (32, 64), (31, 65)], 0.0, [5.0, 5.0, 5.0, 5.0, 5.5],
                    [True, False, True, False, True]))
    out.append(("corner", [(0, 0), (0, 1), (1, 0), (1, 1)], 0.0, [6.0] * 4, [True] * 4))
    out.append(("far_corner", [(H - 1, W - 1), (H - 1, W - 2), (H - 2, W - 1)], 0.0, [7.0, 7.0, 7.0], [True] * 3))
    return out


def gen_heat(shape, a, seed, device):
    """head [B, H, W, Cp]: heat-map logits ~ N(0, 2^2) with every finite bf16 value among them, NaN in every other channel; the
    heat_plateaus blocks (a 1-cell ring of the ring value around each) in class (b + i) % nc of image b"""
    B, H, W, Cp = shape
    c0, nc = a["c0"], a["num_classes"]
    g = _gen(seed, device)
    head = bf16_nan((B, H, W, Cp), device)
    x = _randn((B, H, W, nc), g, device, std=2.0)
    planted = []
    free = torch.ones(x.shape, dtype=torch.bool, device=device)
    for b in range(B):
        for i, (name, cells, ring, vals, peak) in enumerate(heat_plateaus(H, W)):
            c = (b + i) % nc
            for (y, xx) in cells:
                free[b, max(y - 2, 0):y + 3, max(xx - 2, 0):xx + 3, c] = False
                x[b, max(y - 1, 0):y + 2, max(xx - 1, 0):xx + 2, c] = ring
            for (y, xx), v in zip(cells, vals):
                x[b, y, xx, c] = v
            planted.append((b, c, name, cells, peak))
    x = x.to(torch.bfloat16)
    idx = free.reshape(-1).nonzero()[:, 0]
    vals = x.reshape(-1)[idx]
    pos = _spread_all_bf16(vals, g, device)
    x.view(-1)[idx] = vals
    head[..., c0:c0 + nc] = x
    return [head], dict(planted=planted, all_bf16=pos is not None)


def gen_assemble(shapes, seed, device):
    """top_score [B, K] (descending), top_ind2 [B, K] (in [0, C K), 0 and C K - 1 planted), cls_inds [B, C, K] (in [0, H W), 0 and
    H W - 1 planted), wh [B, 2, H, W] (|N(0, 20^2)|), reg [B, 2, H, W] (uniform [0, 1))"""
    (B, K), _, (_, C, _), (_, _, H, W) = shapes[0], shapes[1], shapes[2], shapes[3]
    g = _gen(seed, device)
    ts = torch.rand((B, K), generator=g, device=device).sort(1, descending=True).values
    ti = _randint(0, C * K, (B, K), g, device).to(torch.int32)
    ti[:, 0], ti[:, -1] = 0, C * K - 1
    ci = _randint(0, H * W, (B, C, K), g, device).to(torch.int32)
    ci[:, 0, 0], ci[:, -1, -1] = 0, H * W - 1
    wh = _randn((B, 2, H, W), g, device, std=20.0).abs()
    reg = torch.rand((B, 2, H, W), generator=g, device=device)
    return [ts, ti, ci, wh, None if shapes[4] is None else reg], {}


CP_MOD = 211     # planted CenterPoint cells: r % CP_MOD (ties, saturation, rot (0, 0), z edges)


def gen_centerpoint(shape, a, seed, device):
    """head [B, H, W, C]: NaN outside the task's channels; hm ~ N(logit(score_threshold), 2^2) with every finite bf16 value among the hm
    logits; reg ~ U[0, 1), height ~ N(0, 4^2) (|z| > 10 leaves the range), dim, rot, vel ~ N(0, 1).  Planted cells (hm 3.0 where the
    range decides): r % CP_MOD == 5 equal hm logits (label 0); 9: hm 17, 18 (fp32 sigmoids tie at 1.0); 13: rot (0, 0); 17 / 19 / 23:
    z = 10, -10 (inside: the test is inclusive) and 10.0625 (outside); four cells per image next to the map's centre: the centre on the
    x max / x min / y max / y min edge of post_center_range (reg = the edge's cell offset, exact in bf16 for cells this far from the
    border), the either-outcome decisions of the range test."""
    B, H, W, C = shape
    ncls = a["num_classes"]
    g = _gen(seed, device)
    x = torch.full((B, H * W, C), float("nan"), device=device)
    n = B * H * W

    def fill(off, cnt, t):
        x[..., off:off + cnt] = t.view(B, H * W, cnt)

    fill(a["off_hm"], ncls, _randn((n, ncls), g, device, mean=logit(f32(a["score_threshold"])), std=2.0))
    fill(a["off_reg"], 2, torch.rand((n, 2), generator=g, device=device))
    fill(a["off_height"], 1, _randn((n, 1), g, device, std=4.0))
    fill(a["off_dim"], 3, _randn((n, 3), g, device))
    fill(a["off_rot"], 2, _randn((n, 2), g, device))
    if a["off_vel"] >= 0:
        fill(a["off_vel"], 2, _randn((n, 2), g, device))
    xf = x.view(n, C)
    r = torch.arange(n, device=device)
    loc = r % (H * W)
    gx, gy = loc % W, loc // W
    hm = slice(a["off_hm"], a["off_hm"] + ncls)
    osf, vx, vy = f32(a["out_size_factor"]), f32(a["voxel_size"][0]), f32(a["voxel_size"][1])
    px, py = f32(a["pc_range"][0]), f32(a["pc_range"][1])
    pr = [f32(v) for v in a["post_center_range"]]
    edges = []
    for k, (axis, edge) in enumerate(((0, pr[3]), (0, pr[0]), (1, pr[4]), (1, pr[1]))):
        s = torch.zeros(n, dtype=torch.bool, device=device)
        s[torch.arange(B, device=device) * H * W + (H // 2) * W + W // 2 + k] = True       # one cell per image, near the map's centre
        gc = (gx if axis == 0 else gy)[s].double()
        t = (edge - (px if axis == 0 else py)) / (osf * (vx if axis == 0 else vy)) - gc     # the reg that puts the centre on the edge
        xf[s, a["off_reg"] + axis] = t.float()
        xf[s, hm] = 3.0
        xf[s, a["off_height"]] = 0.0
        edges.append(s.nonzero()[:, 0])
    free_edge = torch.ones(n, dtype=torch.bool, device=device)
    for e in edges:
        free_edge[e] = False
    s = free_edge & (r % CP_MOD == 5)
    xf[s, hm] = 1.0
    s = free_edge & (r % CP_MOD == 9)
    xf[s, hm] = torch.tensor([17.0, 18.0, 19.0][:ncls], device=device) if ncls > 1 else 18.0
    s = free_edge & (r % CP_MOD == 13)
    xf[s, a["off_rot"]:a["off_rot"] + 2] = 0.0
    for m, z in ((17, 10.0), (19, -10.0), (23, 10.0625)):
        s = free_edge & (r % CP_MOD == m)
        xf[s, a["off_height"]] = z
        xf[s, hm] = 3.0
    head = x.view(B, H, W, C).to(torch.bfloat16)
    hmv = head.view(n, C)[:, hm].clone().reshape(-1)
    keep = torch.ones((n, ncls), dtype=torch.bool, device=device)
    keep[(r % CP_MOD == 5) | (r % CP_MOD == 9) | (r % CP_MOD == 17) | (r % CP_MOD == 19) | (r % CP_MOD == 23)] = False
    for e in edges:
        keep[e] = False
    free = keep.reshape(-1).nonzero()[:, 0]
    pos = None
    if free.numel() >= N_BF16_FINITE:
        pos = free[torch.randperm(free.numel(), generator=g, device=device)[:N_BF16_FINITE]]
        hmv[pos] = all_finite_bf16(device)
    head.view(n, C)[:, hm] = hmv.view(n, ncls)
    return [head], dict(edges=edges, all_bf16=pos is not None)
