"""The contract (include/minddet_hip.h) of the kernels that move activations and candidates between the conv, decode, top-k and NMS
stages, in plain torch on float64 / integer tensors: md_maxpool2d, md_sppf_pool, md_upsample_add, md_slice_cast, md_nhwc_to_nchw_f32,
md_concat_copy, md_upsample2x, md_rpn_merge, md_make_rois, md_gather_rows and md_pack_detections -- a reference of every output and the
data generators of tests/test_move_production_gpu.py.  Shared with tests/test_move_reference_cpu.py (the references against
torch.nn.functional / plain Python loops, and what each generator plants).  Pattern: tests/decode_contract.py.

Every operation has an exact answer, so there is no error model:

* copies and casts (md_slice_cast, md_nhwc_to_nchw_f32, md_concat_copy, md_upsample2x, md_rpn_merge, md_make_rois, md_gather_rows,
  md_pack_detections) are compared as BIT PATTERNS: a bf16 -> fp32 cast is `bits << 16`, a copy carries -0, denormals and NaN payloads
  unchanged.  References return int32 bit patterns (`bits16` of a bf16 tensor, `bits32` of an fp32 one).
* the max kernels (md_maxpool2d, md_sppf_pool) are compared as NUMBERS (float64 ==): the header leaves the sign of a zero result
  open (-0 == +0) and NaN inputs unspecified, so the generators keep NaN out of what those kernels read.
* md_upsample_add is one fp32 add and one round-to-nearest-even to bf16, compared as bits.  The reference adds in float64 and rounds
  once.  float64 holds the sum of two bf16 values exactly when their exponents differ by at most 45; past that -- and likewise in the
  step through fp32 that `bf16_rne_bits` takes -- the smaller operand lies below 2^-17 of the larger, while a bf16 rounding boundary
  of the result is at least 2^-9 of it away from the larger operand (8 significant bits), so the extra rounding cannot move the sum
  across a boundary or onto a tie.  Sums with exponents within 16 of each other have at most 24 significant bits: exact in fp32.
  Results below 2^-126 are bf16 denormals (gradual underflow, what torch's conversion does): every such sum is a multiple of 2^-133
  and therefore exact.  The MI355X does not flush them (v_add_f32 and v_cvt_pk_bf16_f32 under the build's default denormal mode): the
  comparison makes no exception for them, and the GPU test asserts that it met as many as the generator planted.

Generators are seeded and take the recorded shapes and attributes; each returns (inputs, plants), plants counting the planted cases
so that tests/test_move_reference_cpu.py fails when a generator stops covering one."""
import numpy as np
import torch

FLT_MAX = float(np.finfo(np.float32).max)
SENT32 = 0x7FA5A5A5        # what outputs start as: an fp32 NaN bit pattern no generator emits
SENT16 = 0x7FA5            # the same for bf16 outputs
POISON32 = 0x7FB7C3D1      # fp32 NaN in source elements the op must not read
POISON16 = 0x7FB7          # bf16 NaN in source channels the op must not read
POISON_LABEL = 0x7FB7C3D1  # int32 label of a source row the op must not read
BF16_MAX_BITS = 0x7F7F
TINY = 2.0 ** -126


def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# bit patterns
# ---------------------------------------------------------------------------------------------------------------------------------
def bits16(x):
    """bf16 tensor -> int32 tensor of its bit patterns, 0 .. 65535"""
    return x.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def from_bits16(b):
    """int tensor of bit patterns 0 .. 65535 -> bf16 tensor"""
    b = b.to(torch.int32)
    return torch.where(b >= 32768, b - 65536, b).to(torch.int16).view(torch.bfloat16)


def bits32(x):
    """fp32 / int32 tensor -> int32 tensor of its bit patterns"""
    return x.contiguous().view(torch.int32)


def f32_from_bits(b):
    return b.to(torch.int32).contiguous().view(torch.float32)


def cast_bits(b16):
    """bit patterns of float(bf16): bits << 16, as (wrapped) int32"""
    v = b16.to(torch.int64) << 16
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


def bf16_rne_bits(s):
    """float64 -> bit patterns of the nearest bf16, ties to even, gradual underflow, overflow to inf (no NaN input)"""
    assert not bool(torch.isnan(s).any())
    u = s.to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF     # innocuous for bf16 + bf16: see above
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).to(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------------
def pool_out(h, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1


def maxpool(x, k, stride, pad, zero_pad):
    """x[N,H,W,C] (bf16 or float64, no NaN) -> float64 y[N,Ho,Wo,C]: the max over the window's in-image taps; with zero_pad a window
    that reaches past the image also competes with 0.  pad < k: every window has an in-image tap."""
    assert 0 <= pad < k and stride >= 1
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H, k, stride, pad), pool_out(W, k, stride, pad)
    xd = x.double()
    assert not bool(torch.isnan(xd).any())
    ninf = float("-inf")
    y = torch.full((N, Ho, Wo, C), ninf, dtype=torch.float64, device=x.device)
    ho, wo = torch.arange(Ho, device=x.device), torch.arange(Wo, device=x.device)
    out_h = torch.zeros(Ho, dtype=torch.bool, device=x.device)
    out_w = torch.zeros(Wo, dtype=torch.bool, device=x.device)
    for dy in range(k):
        hi = ho * stride - pad + dy
        okh = (hi >= 0) & (hi < H)
        out_h |= ~okh
        for dx in range(k):
            wi = wo * stride - pad + dx
            okw = (wi >= 0) & (wi < W)
            out_w |= ~okw
            tap = xd[:, hi.clamp(0, H - 1)][:, :, wi.clamp(0, W - 1)]
            ok = (okh[:, None] & okw[None, :])[None, :, :, None]
            y = torch.maximum(y, torch.where(ok, tap, torch.full_like(tap, ninf)))
    if zero_pad:
        touched = (out_h[:, None] | out_w[None, :])[None, :, :, None]
        y = torch.where(touched, y.clamp_min(0.0), y)
    return y


def sppf(x, k):
    """x = buf[..., 0:C] -> the float64 values of buf[..., C:2C], [2C:3C], [3C:4C]: three chained k x k / 1 / k//2 pools"""
    y1 = maxpool(x, k, 1, k // 2, 0)
    y2 = maxpool(y1, k, 1, k // 2, 0)
    return y1, y2, maxpool(y2, k, 1, k // 2, 0)


def nearest_index(n_out, n_in, device):
    """floor(i * n_in / n_out) in integers"""
    return (torch.arange(n_out, device=device, dtype=torch.int64) * n_in) // n_out


def upsample_add_sum(lat, top):
    """float64 lat + top[n, floor(h Ht / H), floor(w Wt / W)]"""
    H, W, Ht, Wt = lat.shape[1], lat.shape[2], top.shape[1], top.shape[2]
    hi, wi = nearest_index(H, Ht, lat.device), nearest_index(W, Wt, lat.device)
    return lat.double() + top.double()[:, hi][:, :, wi]


def upsample_add(lat, top):
    """-> (bf16 bit patterns of the result, mask of the results below 2^-126)"""
    s = upsample_add_sum(lat, top)
    return bf16_rne_bits(s), (s != 0) & (s.abs() < TINY)


def slice_cast(x, c0, width):
    """x[..., C] bf16 -> fp32 bit patterns of x[..., c0:c0+width]"""
    return cast_bits(bits16(x)[..., c0:c0 + width])


def nhwc_to_nchw_f32(x, c0, width):
    return cast_bits(bits16(x)[..., c0:c0 + width]).permute(0, 3, 1, 2).contiguous()


def concat_copy(src):
    """the bit patterns dst[..., c0:c0+C] receives"""
    return bits16(src)


def upsample2x(src, src_c0, width):
    """the bit patterns dst[n, h, w, c0 + c] = src[n, h // 2, w // 2, src_c0 + c] receives"""
    b = bits16(src)[..., src_c0:src_c0 + width]
    hi = torch.arange(2 * src.shape[1], device=src.device) // 2
    wi = torch.arange(2 * src.shape[2], device=src.device) // 2
    return b[:, hi][:, :, wi]


def rpn_merge(boxes, scores, keep):
    """boxes[L,B,k,4], scores[L,B,k], keep[L,B,k] u8 -> bit patterns of mboxes[B,L*k,4], mscores[B,L*k] (-FLT_MAX where keep == 0)"""
    L, B, k = scores.shape
    mb = bits32(boxes).view(L, B, k, 4).permute(1, 0, 2, 3).reshape(B, L * k, 4)
    fill = bits32(torch.full_like(scores, -FLT_MAX))
    ms = torch.where(keep.view(L, B, k) != 0, bits32(scores), fill).permute(1, 0, 2).reshape(B, L * k)
    return mb, ms


def make_rois(mboxes, topv, topi, cnt):
    """-> bit patterns of rois[B*post,5] (batch index, box; a zero box past cnt) and roi_scores[B*post] (0 past cnt)"""
    B, post = topv.shape
    valid = torch.arange(post, device=topv.device)[None, :] < cnt.view(B, 1)
    idx = torch.where(valid, topi.view(B, post), torch.zeros_like(topi.view(B, post))).long()
    box = torch.gather(bits32(mboxes), 1, idx[:, :, None].expand(B, post, 4))
    box = torch.where(valid[:, :, None], box, torch.zeros_like(box))
    bidx = bits32(torch.arange(B, device=topv.device, dtype=torch.float32))[:, None, None].expand(B, post, 1)
    sc = torch.where(valid, bits32(topv), torch.zeros_like(bits32(topv)))
    return torch.cat([bidx, box], 2).reshape(B * post, 5), sc.reshape(B * post)


def gather_rows(src, idx, cnt):
    """src[B,n,W] f32, idx[B,k], cnt[B] or None -> bit patterns of out[B,k,W] (zero rows past cnt)"""
    B, k = idx.shape
    W = src.shape[2]
    valid = torch.ones((B, k), dtype=torch.bool, device=src.device) if cnt is None else \
        torch.arange(k, device=src.device)[None, :] < cnt.view(B, 1)
    ix = torch.where(valid, idx, torch.zeros_like(idx)).long()
    out = torch.gather(bits32(src), 1, ix[:, :, None].expand(B, k, W))
    return torch.where(valid[:, :, None], out, torch.zeros_like(out))


def pack_detections(boxes, scores, labels, keep_idx, num, max_det, sel_cnt=None, status=None):
    """-> bit patterns of dets[B,max_det,6], count[B], status[B] after the call (None in the 7-parameter form)"""
    B, npre = scores.shape
    n = num.view(B).clamp(max=max_det)
    valid = torch.arange(max_det, device=scores.device)[None, :] < n[:, None]
    # keep_idx may be shorter or longer than max_det: slots past npre are never valid (n <= num <= npre)
    kq = torch.zeros((B, max_det), dtype=torch.int64, device=scores.device)
    m = min(max_det, npre)
    kq[:, :m] = keep_idx.view(B, npre)[:, :m].long()
    q = torch.where(valid, kq, torch.zeros_like(kq))
    bx = torch.gather(bits32(boxes).view(B, npre, 4), 1, q[:, :, None].expand(B, max_det, 4))
    sc = torch.gather(bits32(scores), 1, q)
    lb = bits32(torch.gather(labels.view(B, npre), 1, q).to(torch.float32))
    d = torch.cat([bx, sc[:, :, None], lb[:, :, None]], 2)
    d = torch.where(valid[:, :, None], d, torch.zeros_like(d))
    st = None
    if status is not None:
        flag = (num.view(B) < max_det) & (sel_cnt.view(B) >= npre)
        st = status | flag.to(status.dtype)
    return d, n.to(torch.int32), st


# ---------------------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------------------
def _bf(v):
    return torch.tensor(v, dtype=torch.float32).to(torch.bfloat16)


def pool_border_windows(H, W, k, stride, pad):
    """output windows that reach past the image on each side: dict side -> count (corners: both a row and a column side)"""
    Ho, Wo = pool_out(H, k, stride, pad), pool_out(W, k, stride, pad)
    top = sum(1 for o in range(Ho) if o * stride - pad < 0)
    bot = sum(1 for o in range(Ho) if o * stride - pad + k - 1 >= H)
    lef = sum(1 for o in range(Wo) if o * stride - pad < 0)
    rig = sum(1 for o in range(Wo) if o * stride - pad + k - 1 >= W)
    return dict(top=top * Wo, bottom=bot * Wo, left=lef * Ho, right=rig * Ho, tl=top * lef, tr=top * rig, bl=bot * lef, br=bot * rig)


def gen_pool(shape, a, seed, device, sppf_radius=0):
    """x[N,H,W,C] bf16 for md_maxpool2d (a = dict(k, stride, pad, zero_pad)) or, with sppf_radius = k // 2, channels [0, C) of an
    md_sppf_pool buffer.  No NaN.  Channel c % 8 of every image carries:
      0  negative values only: every window that touches the padding has all its in-image taps negative (zero_pad decides)
      1  a dominating maximum (1024 + 8 t) at tap t = (dy, dx) of its own window, for each of the k x k taps that fit
      2  plateaus: blocks of one constant (equal maxima) among smaller values
      3  zeros of both signs, and -0 among negative values
      4  +inf and -inf, single and in blocks (a window of -inf only)
      5  the largest finite bf16 of both signs, the smallest normals and the smallest denormals of both signs
      6  SPPF: distinct maxima at the four image corners, and one at an interior pixel: it must reach exactly 3R along its row and column
      7  Gaussian
    plants: border (pool_border_windows), taps, plateau, zeros, infs, extremes, corners, far"""
    N, H, W, C = shape
    k, s, p = a["k"], a["stride"], a["pad"]
    g = _gen(seed, device)
    x = (2.0 * torch.randn((N, H, W, C), generator=g, device=device)).to(torch.bfloat16)
    pl = dict(border=pool_border_windows(H, W, k, s, p), taps=0, plateau=0, zeros=0, infs=0, extremes=0, corners=0, far=0)
    if x.numel() == 0:
        return [x], pl
    x[..., 0::8] = -(x[..., 0::8].abs() + 0.0078125)
    Ho, Wo = pool_out(H, k, s, p), pool_out(W, k, s, p)
    step, base = (k + s - 1) // s + 1, (p + s - 1) // s
    for t in range(k * k):               # window (ho, wo) of tap t: windows of different taps do not overlap
        ho, wo = base + (t // k) * step, base + (t % k) * step
        hi, wi = ho * s - p + t // k, wo * s - p + t % k
        if ho < Ho and wo < Wo and hi < H and wi < W:
            x[:, hi, wi, 1::8] = 1024.0 + 8 * t
            pl["taps"] += 1
    for j in range(3):                   # plateaus of k + 1 pixels square, clipped at the image
        h0, w0 = (j * (H // 3)) % max(H, 1), (j * (W // 2)) % max(W, 1)
        x[:, h0:h0 + k + 1, w0:w0 + k + 1, 2::8] = 7.0 + j
        pl["plateau"] += 1
    zb = torch.where(torch.rand((N, H, W), generator=g, device=device) < 0.5, 0, 0x8000)
    negv = bits16((-(torch.randn((N, H, W), generator=g, device=device).abs() + 0.0078125)).to(torch.bfloat16))
    neg = torch.rand((N, H, W), generator=g, device=device) < 0.5
    neg[:, :H // 2] = False                                              # upper half: zeros only; lower half: zeros among negatives
    zb = torch.where(neg, negv, zb)
    x[..., 3::8] = from_bits16(zb)[..., None]
    pl["zeros"] = min(int((zb == 0x8000).sum()), int((zb == 0).sum()))
    r = torch.rand((N, H, W), generator=g, device=device)
    c4 = torch.where(r[..., None] > 0.9, float("-inf"), x[..., 4::8].float())
    x[..., 4::8] = torch.where(r[..., None] < 0.02, float("inf"), c4).to(torch.bfloat16)
    x[:, :min(H, 2 * k), :min(W, 2 * k), 4::8] = float("-inf")           # a block of -inf: windows that hold nothing else
    pl["infs"] = int(torch.isinf(x[..., 4::8]).sum())
    ext = torch.tensor([0x7F7F, 0xFF7F, 0x0080, 0x8080, 0x0001, 0x8001, 0x0000], device=device)
    e = ext[torch.randint(0, len(ext), (N, H, W), generator=g, device=device)]
    x[..., 5::8] = from_bits16(e)[..., None]
    pl["extremes"] = int(torch.unique(e).numel())
    if sppf_radius:
        R3 = 3 * sppf_radius
        x[..., 6::8] = (x[..., 6::8].float().clamp(-4, 4)).to(torch.bfloat16)
        for j, (h, w) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
            x[:, h, w, 6::8] = 2048.0 + 16 * j
            pl["corners"] += 1
        hc, wc = H // 2, W // 2          # interior: lower than the corners' values, so visible only where no corner reaches
        if hc - R3 >= 0 and wc - R3 >= 0 and hc + R3 < H and wc + R3 < W:
            pl["far"] = 1
        x[:, hc, wc, 6::8] = 512.0
    return [x], pl


def gen_upsample_add(shapes, seed, device):
    """lat[N,H,W,C], top[N,Ht,Wt,C] bf16: Gaussian values (normal numbers, no NaN / inf / denormal input) and, against the top value
    each lateral element meets, planted laterals: exact bf16 ties of the fp32 sum (even and odd neighbour below), sums that overflow
    to +inf and -inf, sums that cancel to zero and sums below 2^-126.
    plants: tie_even, tie_odd, overflow_pos, overflow_neg, cancel, subnormal (counted on the float64 sum of the returned tensors)"""
    (N, H, W, C), (_, Ht, Wt, _) = shapes[0], shapes[1]
    g = _gen(seed, device)
    top = (3.0 * torch.randn((N, Ht, Wt, C), generator=g, device=device)).to(torch.bfloat16)
    lat = (3.0 * torch.randn((N, H, W, C), generator=g, device=device)).to(torch.bfloat16)
    pl = dict(tie_even=0, tie_odd=0, overflow_pos=0, overflow_neg=0, cancel=0, subnormal=0)
    if lat.numel() == 0:
        return [lat, top], pl
    tb = bits16(top)
    r = torch.rand(tb.shape, generator=g, device=device)
    m = torch.randint(0, 128, tb.shape, generator=g, device=device, dtype=torch.int32)
    sign = tb & 0x8000
    tb = torch.where(r < 0.01, sign | BF16_MAX_BITS, tb)                                 # +-max: the lateral adds max again
    tb = torch.where((r >= 0.01) & (r < 0.03), sign | ((127 - 120) << 7) | m, tb)        # +-2^-120 (1 + m / 128)
    tb = torch.where((tb & 0x7F80) == 0, sign | (100 << 7) | m, tb)                        # no zero / denormal input
    top = from_bits16(tb)
    hi, wi = nearest_index(H, Ht, device), nearest_index(W, Wt, device)
    t = tb[:, hi][:, :, wi]
    ts, te, tm = t & 0x8000, (t >> 7) & 0xFF, t & 0x7F
    lb = bits16(lat)
    lb = torch.where((lb & 0x7F80) == 0, (lb & 0x8000) | (101 << 7) | (lb & 0x7F), lb)
    u = torch.rand(t.shape, generator=g, device=device)
    big, tiny = (t & 0x7FFF) == BF16_MAX_BITS, te == 7
    lb = torch.where(big, t, lb)                                                         # max + max -> inf
    lb = torch.where(tiny, (ts ^ 0x8000) | (7 << 7) | torch.where(tm < 127, tm + 1, tm - 1), lb)   # difference 2^-127
    plain = ~big & ~tiny
    lb = torch.where(plain & (u < 0.03) & (te > 9), ts | ((te - 8) << 7), lb)            # t + sign(t) 2^(e-8): an exact tie
    lb = torch.where(plain & (u >= 0.03) & (u < 0.04), t ^ 0x8000, lb)                   # t - t
    lat = from_bits16(lb)
    s = upsample_add_sum(lat, top)
    f = s.to(torch.float32).contiguous().view(torch.int32)
    tie = ((f & 0xFFFF) == 0x8000) & torch.isfinite(s)
    pl.update(tie_even=int((tie & (((f >> 16) & 1) == 0)).sum()), tie_odd=int((tie & (((f >> 16) & 1) == 1)).sum()),
              overflow_pos=int((s >= 2.0 ** 128).sum()), overflow_neg=int((s <= -2.0 ** 128).sum()), cancel=int((s == 0).sum()),
              subnormal=int(((s != 0) & (s.abs() < TINY)).sum()))
    return [lat, top], pl


def gen_patterns(shape, c0, width, seed, device):
    """x[..., Cs] bf16 for a copy or a cast that reads channels [c0, c0 + width): random bit patterns there -- every one of the 65536
    (NaN payloads, infinities, denormals, both zeros) when the slice holds that many elements -- and POISON16 in every other channel.
    plants: patterns (distinct patterns in the slice), poison (poisoned elements)"""
    g = _gen(seed, device)
    b = torch.full(tuple(shape), POISON16, dtype=torch.int32, device=device)
    lead = 1
    for s_ in shape[:-1]:
        lead *= s_
    n = lead * width
    v = torch.randint(0, 65536, (n,), generator=g, device=device, dtype=torch.int32)
    if n >= 65536:
        pos = torch.randperm(n, generator=g, device=device)[:65536]
        v[pos] = torch.arange(65536, dtype=torch.int32, device=device)
    if n:
        b.view(lead, shape[-1])[:, c0:c0 + width] = v.view(lead, width)
    pl = dict(patterns=int(torch.unique(v).numel()), poison=int(b.numel() - n))
    return [from_bits16(b)], pl


_SPECIAL32 = [0x80000000, 0x00000000, 0xFF7FFFFF, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7FC01234, 0xFFC00001, 0x00000001, 0x80000001]


def _rows32(shape, g, device, scale=100.0):
    """fp32 data of copies: Gaussian values with the special bit patterns (-0, -FLT_MAX, infinities, NaN payloads, denormals) strewn in"""
    x = scale * torch.randn(tuple(shape), generator=g, device=device)
    if x.numel():
        sp = torch.tensor([v - (1 << 32) if v >= (1 << 31) else v for v in _SPECIAL32], dtype=torch.int32, device=device)
        pick = torch.randint(0, len(sp), tuple(shape), generator=g, device=device)
        x = torch.where(torch.rand(tuple(shape), generator=g, device=device) < 0.05, f32_from_bits(sp[pick]), x)
    return x


def _wrap32(v):
    return v - (1 << 32) if v >= (1 << 31) else v


def gen_rpn_merge(shapes, seed, device):
    """boxes[L,B,k,4], scores[L,B,k] fp32 (-0, -FLT_MAX and NaN payloads among them), keep[L,B,k] u8 drawn from 0, 1, 2, 255.
    plants: keep (distinct keep bytes), neg_zero, neg_fltmax (scores with that pattern)"""
    L, B, k = shapes[1]
    g = _gen(seed, device)
    boxes, scores = _rows32((L, B, k, 4), g, device), _rows32((L, B, k), g, device, 1.0)
    kv = torch.tensor([0, 1, 2, 255], dtype=torch.uint8, device=device)
    keep = kv[torch.randint(0, 4, (L, B, k), generator=g, device=device)]
    sb = bits32(scores)
    pl = dict(keep=int(torch.unique(keep).numel()), neg_zero=int((sb == _wrap32(0x80000000)).sum()),
              neg_fltmax=int((sb == _wrap32(0xFF7FFFFF)).sum()))
    return [boxes, scores, keep], pl


COUNT_KINDS = 4      # 0, 1, partial, full


def _counts(B, full, device, shift=0):
    """[B] int32 cycling through 0, 1, a partial count and `full`"""
    c = [(0, 1, max(full // 2, 0), full)[(i + shift) % COUNT_KINDS] for i in range(B)]
    return torch.tensor(c, dtype=torch.int32, device=device).clamp(max=full)


def _indices(B, k, n, cnt, g, device):
    """idx[B,k] int32 into n source rows, and the poisoned row (or -1 when n < 3).  Valid slots (j < cnt[b]): slot 0 holds row 0, the
    last valid slot row n - 1, slots 1 and 2 the same row (a repeat), the others random rows; none is the poisoned row n // 2.  Every
    slot past cnt[b] holds the poisoned row: in range, so a kernel that reads it returns NaN and does not fault."""
    poison = n // 2 if n >= 3 else -1
    idx = torch.randint(0, max(n, 1), (B, k), generator=g, device=device, dtype=torch.int32)
    if poison >= 0:
        idx = torch.where(idx == poison, torch.zeros_like(idx), idx)
    j = torch.arange(k, device=device)[None, :]
    c = cnt.view(B, 1)
    if k >= 3:
        idx[:, 2] = idx[:, 1]
    if k >= 1:
        idx[:, 0] = 0
    idx = torch.where(j == c - 1, torch.full_like(idx, max(n - 1, 0)), idx)
    idx = torch.where(j >= c, torch.full_like(idx, max(poison, 0)), idx)
    return idx, poison


def gen_make_rois(shapes, seed, device):
    """mboxes[B,P,4], topv[B,post], topi[B,post], cnt[B]: counts 0, 1, partial, full; indices as _indices; the poisoned box row and every
    topv slot past cnt are POISON32.  plants: counts (distinct kinds), poison_slots (slots past cnt that point at the poisoned row)"""
    (B, P, _), (_, post) = shapes[0], shapes[1]
    g = _gen(seed, device)
    cnt = _counts(B, post, device)
    mboxes, topv = _rows32((B, P, 4), g, device), _rows32((B, post), g, device, 1.0)
    topi, poison = _indices(B, post, P, cnt, g, device)
    past = torch.arange(post, device=device)[None, :] >= cnt.view(B, 1)
    if poison >= 0:
        mboxes[:, poison] = f32_from_bits(torch.tensor(POISON32, device=device))
    topv = torch.where(past, f32_from_bits(torch.full((B, post), POISON32, dtype=torch.int32, device=device)), topv)
    pl = dict(counts=len(set(cnt.tolist())), poison_slots=int(past.sum()) if poison >= 0 else 0, first=int((topi == 0).any()) if B else 0,
              last=int(((topi == P - 1) & ~past).any()) if B else 0)
    return [mboxes, topv, topi, cnt], pl


def gen_gather_rows(shapes, with_cnt, seed, device):
    """src[B,n,W], idx[B,k], cnt[B] or None (then every slot is valid and no row is poisoned)"""
    (B, n, W), (_, k) = shapes[0], shapes[1]
    g = _gen(seed, device)
    cnt = _counts(B, k, device) if with_cnt else torch.full((B,), k, dtype=torch.int32, device=device)
    src = _rows32((B, n, W), g, device)
    idx, poison = _indices(B, k, n, cnt, g, device)
    past = torch.arange(k, device=device)[None, :] >= cnt.view(B, 1)
    if poison >= 0 and with_cnt:
        src[:, poison] = f32_from_bits(torch.tensor(POISON32, device=device))
    pl = dict(counts=len(set(cnt.tolist())), poison_slots=int(past.sum()) if poison >= 0 else 0, first=int((idx == 0).any()) if B else 0,
              last=int(((idx == n - 1) & ~past).any()) if B else 0)
    return [src, idx, cnt if with_cnt else None], pl


NUM_KINDS, SEL_KINDS, STATUS_KINDS = 6, 3, 4
PACK_COMBOS = NUM_KINDS * SEL_KINDS * STATUS_KINDS
STATUS_VALUES = (0, 1, 2, 0x7FFFFFFE)


def pack_phases(B):
    """how many generator phases cover every (num, sel_cnt, status) combination at batch B"""
    return (PACK_COMBOS + B - 1) // B if B else 1


def gen_pack(shapes, max_det, status_form, seed, device, phase=0):
    """boxes[B,npre,4], scores[B,npre], labels[B,npre], keep_idx[B,npre], num[B] (, sel_cnt[B], status[B]).  Image i of phase p takes
    combination c = p B + i of
      num      0, 1, max_det // 2, max_det - 1, max_det, above max_det (each capped at npre)
      sel_cnt  0, npre - 1, npre
      status   0, 1, 2, 0x7ffffffe
    so pack_phases(B) phases hold all four outcomes of (num < max_det, sel_cnt >= npre), both boundaries and every status word.
    keep_idx as _indices against min(num, max_det); the poisoned row (boxes, scores POISON32, label POISON_LABEL) sits in every slot past it.
    plants: combos (the set of (num < max_det, sel_cnt >= npre) pairs), num_eq, sel_below (boundary counts), status (distinct words)"""
    B, npre = shapes[1]
    g = _gen(seed, device)
    nums, sels, stats = [], [], []
    for i in range(B):
        c = phase * B + i
        nums.append(min((0, 1, max_det // 2, max_det - 1, max_det, max_det + 3)[c % NUM_KINDS], npre))
        sels.append((0, npre - 1, npre)[(c // NUM_KINDS) % SEL_KINDS])
        stats.append(STATUS_VALUES[(c // (NUM_KINDS * SEL_KINDS)) % STATUS_KINDS])
    num = torch.tensor(nums, dtype=torch.int32, device=device).view(B)
    sel = torch.tensor(sels, dtype=torch.int32, device=device).view(B)
    status = torch.tensor(stats, dtype=torch.int32, device=device).view(B)
    boxes, scores = _rows32((B, npre, 4), g, device), _rows32((B, npre), g, device, 1.0)
    labels = torch.randint(-1, 91, (B, npre), generator=g, device=device, dtype=torch.int32)
    kidx, poison = _indices(B, npre, npre, num.clamp(max=max_det), g, device)
    if poison >= 0:
        boxes[:, poison] = f32_from_bits(torch.tensor(POISON32, device=device))
        scores[:, poison] = f32_from_bits(torch.tensor(POISON32, device=device))
        labels[:, poison] = POISON_LABEL
    pl = dict(combos={(n < max_det, s >= npre) for n, s in zip(nums, sels)}, num_eq=sum(n == max_det for n in nums),
              num_above=sum(n > max_det for n in nums), sel_below=sum(s == npre - 1 for s in sels), status=set(stats))
    ins = [boxes, scores, labels, kidx, num]
    return (ins + [sel, status] if status_form else ins), pl
