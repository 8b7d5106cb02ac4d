"""The contract of md_pp_scores and md_pp_decode_selected (include/minddet_hip_pp.h) in float64 torch: a reference of every output,
an elementwise bound on how far the kernel's fp32 value may lie from it, and the data generators of tests/test_pointpillars_gpu.py.
Shared with tests/test_pointpillars_cpu.py (the references against the reference-generated vectors, the generators' plants, the
either-outcome cap).  The tracked-value machinery and the error model are tests/decode_contract.py's; this file adds:

* sqrtf is correctly rounded (the build keeps hipcc's default correctly rounded fp32 divide and square root): one rounding, RND,
  on top of the operand's error carried through the square root, e / sqrt(v - e) (sqrt(v) - sqrt(v - e) = e / (sqrt(v) + sqrt(v - e))).
* sinf / cosf: the OpenCL accuracy requirement of 4 ulp (8 u relative) that the device library meets over the whole range, with the
  margin 16 u, plus the TINY floor; both are 1-Lipschitz in the argument.
* fminf / fmaxf over the four corners of a standup box are 1-Lipschitz in every operand: the bound is the largest operand bound.
* The direction fix adds (float)pi where the reference adds pi: the float64 value uses pi, and the bound is charged |pi - (float)pi|
  = 8.74e-8 on top of the one rounding of the sum.

Either-outcome decisions (each function returns how many of its decisions are of that kind; the tests cap the share at CAP):
* the class argmax where another class's float64 score lies within the two bounds of the best one AND its logit differs -- equal
  logits give equal fp32 scores, so an exact tie is NOT of this kind: the lower class must win;
* the direction argmax: its operands are exact bf16 values, so it is never of this kind (counted for the record);
* rot > 0 where |rot| is within its bound: the fix may or may not be applied, both forms are accepted;
* the score against the -1 of a masked anchor: a sigmoid is >= 0, never of this kind (counted for the record)."""
import math

import numpy as np
import torch

from tests.decode_contract import CAP, RND, TINY, U, Expect, T, add, check, d64, decision, div, expf, f32, mul, sigmoid, stack, sub  # noqa: F401

SINCOS = 16 * U                                   # sinf / cosf relative error (4 ulp), with the margin
PI_ERR = abs(math.pi - f32(math.pi))              # |pi - (float)pi|


def sqrtf(a):
    v = torch.sqrt(a.v)
    e = a.e / torch.sqrt((a.v - a.e).clamp(min=TINY))
    return T(v, e + RND * (v + e))


def sinf(a):
    v = torch.sin(a.v)
    return T(v, a.e + SINCOS * v.abs() + TINY)


def cosf(a):
    v = torch.cos(a.v)
    return T(v, a.e + SINCOS * v.abs() + TINY)


def tmin(ts):
    return T(torch.stack([t.v for t in ts]).min(0).values, torch.stack([t.e for t in ts]).max(0).values)


def tmax(ts):
    return T(torch.stack([t.v for t in ts]).max(0).values, torch.stack([t.e for t in ts]).max(0).values)


# ---------------------------------------------------------------------------------------------------------------------------------
# the two device functions of csrc/box_codec.h
# ---------------------------------------------------------------------------------------------------------------------------------
def second_box_decode(enc, anchors):
    """enc [..., 7], anchors [..., 7] (float64 of exact bf16 / fp32 values) -> T [..., 7] = (x, y, z, w, l, h, r): the operation
    sequence of second_box_decode_one"""
    t = [T(enc[..., j]) for j in range(7)]
    xa, ya, za0, wa, la, ha, ra = (T(anchors[..., j]) for j in range(7))
    za = add(za0, div(ha, 2.0))
    diagonal = sqrtf(add(mul(la, la), mul(wa, wa)))
    xg, yg, zg = add(mul(t[0], diagonal), xa), add(mul(t[1], diagonal), ya), add(mul(t[2], ha), za)
    lg, wg, hg = mul(expf(t[4]), la), mul(expf(t[3]), wa), mul(expf(t[5]), ha)
    rg = add(t[6], ra)
    return stack([xg, yg, sub(zg, div(hg, 2.0)), wg, lg, hg, rg])


def standup(cx, cy, dx, dy, r):
    """tracked (x, y, dx, dy, r) -> T [..., 4] = (xmin, ymin, xmax, ymax): the operation sequence of standup_one"""
    s, c = sinf(r), cosf(r)
    qx, qy = [], []
    for nx, ny in ((-0.5, -0.5), (-0.5, 0.5), (0.5, 0.5), (0.5, -0.5)):
        px, py = mul(dx, nx), mul(dy, ny)
        qx.append(add(add(mul(px, c), mul(py, s)), cx))
        qy.append(add(add(mul(mul(px, -1.0), s), mul(py, c)), cy))
    return stack([tmin(qx), tmin(qy), tmax(qx), tmax(qy)])


# ---------------------------------------------------------------------------------------------------------------------------------
# md_pp_scores
# ---------------------------------------------------------------------------------------------------------------------------------
def scores(head, mask, a):
    """head [B,H,W,C] bf16, mask [B,N] (bool / uint8) or None, a = dict(off_cls, num_anchors, num_classes) ->
    (dict(scores=Expect, labels=callable got -> bool ok), n_decisions, n_either)"""
    B, H, W, _ = head.shape
    A, K, off = a["num_anchors"], a["num_classes"], a["off_cls"]
    x = d64(head[..., off:off + A * K]).reshape(B, H * W * A, K)
    s = sigmoid(x)
    best = s.v.max(-1, keepdim=True).values
    ks = torch.arange(K, device=head.device).expand_as(x)
    want = torch.where(s.v == best, ks, torch.full_like(ks, K)).min(-1).values                 # the first class at the maximum
    e_best = torch.gather(s.e, 2, want[..., None])
    x_best = torch.gather(x, 2, want[..., None])
    close = (best - s.v <= e_best + s.e) & (x != x_best)                                        # another logit, overlapping score
    either = close.any(-1)
    val = T(best[..., 0], s.e.max(-1).values)
    live = torch.ones_like(either) if mask is None else mask.reshape(B, -1) != 0
    sure_pos, _ = decision(val, -1.0)                                                           # the score against -1

    def labels_ok(got):
        g = got.long().clamp(0, K - 1)
        return (got.long() == want) | (torch.gather(close, 2, g[..., None])[..., 0] & (got.long() == g))

    out = dict(scores=Expect(val=val, fill=-1.0, want_val=live, want_fill=~live), labels=labels_ok)
    n_dec = (either.numel() if K > 1 else 0) + live.numel()
    return out, n_dec, int(either.sum()) + int((~sure_pos).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# md_pp_decode_selected
# ---------------------------------------------------------------------------------------------------------------------------------
def decode_selected(head, anchors, idx, cnt, sel_scores, labels, a):
    """head [B,H,W,C] bf16, anchors [N,7] f32, idx [B,k] i32, cnt [B] i32, sel_scores [B,k] f32, labels [B,N] i32,
    a = dict(off_box, off_dir, num_anchors) -> (dict(boxes=Expect [B,k,7] before the fix, standup=Expect [B,k,4], rot=callable,
    dir_labels=int64 [B,k], score=[B,k], label=[B,k], live=[B,k]), n_decisions, n_either)"""
    B, H, W, C = head.shape
    A = a["num_anchors"]
    k = idx.shape[1]
    live = torch.arange(k, device=head.device)[None] < cnt[:, None].long()
    ii = torch.where(live, idx.long(), torch.zeros_like(idx.long()))
    cell, an = ii // A, ii % A
    rows = torch.gather(d64(head).reshape(B, H * W, C), 1, cell[..., None].expand(B, k, C))
    enc = torch.stack([torch.gather(rows, 2, (a["off_box"] + an * 7 + j)[..., None])[..., 0] for j in range(7)], -1)
    box = second_box_decode(enc, d64(anchors)[ii])
    st = standup(box[..., 0], box[..., 1], box[..., 3], box[..., 4], box[..., 6])
    zero = lambda t, n: T(torch.where(live[..., None].expand_as(t.v), t.v, torch.zeros_like(t.v)),
                          torch.where(live[..., None].expand_as(t.v), t.e, torch.zeros_like(t.e)))
    box, st = zero(box, 7), zero(st, 4)
    rot = box[..., 6]
    n_dec, n_either = 0, 0
    if a["off_dir"] is not None and a["off_dir"] >= 0:
        d0 = torch.gather(rows, 2, (a["off_dir"] + an * 2)[..., None])[..., 0]
        d1 = torch.gather(rows, 2, (a["off_dir"] + an * 2 + 1)[..., None])[..., 0]
        dirs = (d1 > d0).long() * live.long()
        pos, notpos = decision(rot, 0.0)
        fixed_v = rot.v + math.pi
        fixed = T(fixed_v, rot.e + PI_ERR + RND * (fixed_v.abs() + rot.e + PI_ERR))
        # a sure sign: the fix is applied exactly where (rot > 0) != (dir != 0); an unsure one: both forms are accepted
        may_fix = live & torch.where(pos | notpos, pos != (dirs != 0), torch.ones_like(pos))
        may_keep = torch.where(pos | notpos, pos == (dirs != 0), torch.ones_like(pos)) | ~live
        n_dec = 2 * int(live.sum())
        n_either = int((live & ~(pos | notpos)).sum())
    else:
        dirs = torch.zeros_like(ii)
        fixed, may_fix, may_keep = rot, torch.zeros_like(live), torch.ones_like(live)

    def rot_ok(got):
        g = got.double()
        keep = may_keep & ((g - rot.v).abs() <= rot.e)
        fix = may_fix & ((g - fixed.v).abs() <= fixed.e)
        return keep | fix

    l7, l4 = live[..., None].expand(B, k, 7), live[..., None].expand(B, k, 4)
    lab = torch.gather(labels.long(), 1, ii) * live.long()
    out = dict(boxes=Expect(val=box, fill=0.0, want_val=l7, want_fill=~l7), standup=Expect(val=st, fill=0.0, want_val=l4, want_fill=~l4),
               rot=rot_ok, dir_labels=dirs, score=torch.where(live, sel_scores, torch.zeros_like(sel_scores)), label=lab, live=live,
               rot_fixed=may_fix & ~may_keep)
    return out, n_dec, n_either


# ---------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------
SHAPES = {                      # name: (B, H, W, A, K, C)
    "clamp": (2, 6, 10, 2, 1, 24),        # fewer anchors (120) than nms_pre_max_size: k clamps
    "odd": (3, 31, 33, 4, 2, 48),         # odd sizes, 4 092 anchors > 900, a partial last wave
    "three": (2, 5, 7, 2, 3, 24),         # three classes: the kernel's scalar-load form (K is neither 1 nor 2)
    "car": (4, 248, 216, 2, 1, 24),       # the Car config's head at batch 4
    "ped_cycle": (2, 248, 296, 4, 2, 48),   # the Cyclist / Pedestrian head: the top-k's multi-workgroup form
}
SATURATED = 4                   # planted anchors per sample whose two class logits both saturate the fp32 sigmoid (where 4 of N is under CAP)
TIES = 4                        # planted anchors per sample with exactly equal class logits


def offsets(A, K):
    return dict(off_cls=0, off_box=A * K, off_dir=A * K + A * 7, num_anchors=A, num_classes=K)


def make_head(name, seed=0, device="cpu"):
    """-> (head [B,H,W,C] bf16, attrs, plants).  Class logits are bf16 values in about [-12, 6]; box encodings N(0, 0.5) with the
    angle code kept at least 2^-6 away from 0 (rot = code + the anchor's 0 or 1.57 is then not clustered at 0); direction logits
    N(0, 2), equal on a few anchors.  Planted per sample for K > 1: SATURATED anchors with class logits (24, 30) -- both sigmoids are
    1.0f, float64 prefers class 1 -- and TIES anchors with equal logits."""
    B, H, W, A, K, C = SHAPES[name]
    g = torch.Generator().manual_seed(1000 + seed)
    a = offsets(A, K)
    N = H * W * A
    head = torch.zeros((B, H * W, C), dtype=torch.float32)
    cls = torch.rand((B, N, K), generator=g) * 18.0 - 12.0
    plants = dict(saturated=[], ties=[], dir_ties=[])
    if K > 1:
        for b in range(B):
            n_sat = SATURATED if SATURATED <= CAP * N else 0
            p = torch.randperm(N, generator=g)[:n_sat + TIES]
            cls[b, p, 2:] = -12.0                                              # classes 0 and 1 lead on the planted anchors
            cls[b, p[:n_sat], 0], cls[b, p[:n_sat], 1] = 24.0, 30.0
            cls[b, p[n_sat:], 1] = cls[b, p[n_sat:], 0].bfloat16().float()
            cls[b, p[n_sat:], 0] = cls[b, p[n_sat:], 1]
            plants["saturated"].append(p[:n_sat])
            plants["ties"].append(p[n_sat:])
    head[:, :, :A * K] = cls.reshape(B, H * W, A * K)
    enc = torch.randn((B, N, 7), generator=g) * 0.5
    ang = enc[..., 6]
    enc[..., 6] = torch.where(ang.abs() < 2.0 ** -6, torch.full_like(ang, 0.25), ang)
    head[:, :, a["off_box"]:a["off_box"] + A * 7] = enc.reshape(B, H * W, A * 7)
    dirs = torch.randn((B, N, 2), generator=g) * 2.0
    for b in range(B):
        p = torch.randperm(N, generator=g)[:4]
        dirs[b, p, 1] = dirs[b, p, 0]
        plants["dir_ties"].append(p)
    head[:, :, a["off_dir"]:a["off_dir"] + A * 2] = dirs.reshape(B, H * W, A * 2)
    return head.reshape(B, H, W, C).to(torch.bfloat16).to(device), a, plants


def make_anchors(name, device="cpu"):
    """anchors [N,7] f32 in the layout of the anchor generators: per cell A anchors, rotations 0 and 1.57 alternating, two sizes for
    A = 4; centres on a 0.32 m grid"""
    B, H, W, A, K, C = SHAPES[name]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    out = torch.zeros((H, W, A, 7), dtype=torch.float32)
    sizes = [(1.6, 3.9, 1.56, -1.78)] if A == 2 else [(0.6, 1.76, 1.73, -1.465), (0.6, 0.8, 1.73, -1.2)]
    for i in range(A):
        w, l, h, z = sizes[i // 2]
        out[:, :, i, 0], out[:, :, i, 1], out[:, :, i, 2] = xs * 0.32 + 0.16, ys * 0.32 - 0.16 * H, z
        out[:, :, i, 3], out[:, :, i, 4], out[:, :, i, 5], out[:, :, i, 6] = w, l, h, (0.0, 1.57)[i % 2]
    return out.reshape(-1, 7).to(device)


def make_mask(name, seed=0, device="cpu", all_masked_sample=None):
    """uint8 [B,N], about 70 % valid; all_masked_sample: one sample with no valid anchor"""
    B, H, W, A, K, C = SHAPES[name]
    g = torch.Generator().manual_seed(2000 + seed)
    m = (torch.rand((B, H * W * A), generator=g) < 0.7).to(torch.uint8)
    if all_masked_sample is not None:
        m[all_masked_sample] = 0
    return m.to(device)
