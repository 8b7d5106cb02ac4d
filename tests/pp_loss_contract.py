"""The contract of md_pp_loss / md_pp_loss_grad (include/minddet_hip_pploss.h) in numpy float64: the normaliser, the focal, smooth-L1 and
direction terms, the five parts, total, and the analytic gradient of total with respect to every head element.  Inputs are the values
the operator is given (the bf16 head values widened exactly, the fp32 targets, anchors and attributes); nothing here is rounded.
tests/test_pp_loss_cpu.py compares it with a literal torch-float64 transcription of the reference's loss under autograd;
tests/test_pp_loss_gpu.py holds the device result to it.  ulps_apart and compare_losses are those of
tests/cp_loss_contract.py; compare_grad (its structural zeros are a condition of its own) lives here.  No torch."""
import numpy as np

from tests.cp_loss_contract import compare_losses, ulps_apart  # noqa: F401

DEFAULTS = dict(alpha=0.25, gamma=2.0, sigma=3.0, code_weights=(1.0,) * 7, cls_weight=1.0, loc_weight=2.0, dir_weight=0.2,
                pos_cls_weight=1.0, neg_cls_weight=1.0)


def f32(v):
    """the value an fp32 attribute carries"""
    return float(np.float32(v))


def softplus_sigmoid(s):
    """-> softplus(s) = max(s, 0) + log1p(exp(-|s|)), sigmoid(s), sigmoid(-s); nothing is formed as 1 - sigmoid"""
    e = np.exp(-np.abs(s))
    r = 1.0 / (1.0 + e)
    return np.maximum(s, 0.0) + np.log1p(e), np.where(s >= 0, r, e * r), np.where(s >= 0, e * r, r)


def loss(head, labels, reg_targets, anchors, *, off_cls, off_box, off_dir, num_anchors, num_classes, alpha=0.25, gamma=2.0, sigma=3.0,
         code_weights=(1.0,) * 7, cls_weight=1.0, loc_weight=2.0, dir_weight=0.2, pos_cls_weight=1.0, neg_cls_weight=1.0, with_grad=True):
    """head [B,H,W,C] (float array of the bf16 values; channels no head owns may hold anything), labels [B,N], reg_targets [B,N,7] f32,
    anchors [N,7] f32; off_dir None / -1: no direction loss; alpha None: no alpha factor -> dict of float64: parts [5] (loc, cls, dir,
    cls_pos, cls_neg), num_pos [B], total (scalar), grad [B,H,W,C] and structural [B,H,W,C] bool (the elements the header promises
    to be exactly +0.0)"""
    B, H, W, C = head.shape
    A, K = int(num_anchors), int(num_classes)
    N = H * W * A
    assert labels.shape == (B, N) and reg_targets.shape == (B, N, 7) and anchors.shape == (N, 7)
    has_dir = off_dir is not None and off_dir >= 0
    alpha_pos, alpha_neg = (1.0, 1.0) if alpha is None or alpha < 0 else (f32(alpha), 1.0 - f32(alpha))
    gamma, sigma = f32(gamma), f32(sigma)
    cw = np.array([f32(v) for v in code_weights], np.float64)
    cls_weight, loc_weight, dir_weight = f32(cls_weight), f32(loc_weight), f32(dir_weight)
    pcw, ncw = f32(pos_cls_weight), f32(neg_cls_weight)

    cells = head.reshape(B, H * W, C)
    pos, neg = labels > 0, labels == 0
    num_pos = pos.sum(1).astype(np.float64)
    nb = np.maximum(num_pos, 1.0)[:, None]                                     # [B,1]
    grad = np.zeros((B, H * W, C))
    structural = np.ones((B, H * W, C), bool)

    # classification: every anchor and class
    x = cells[:, :, off_cls:off_cls + A * K].astype(np.float64).reshape(B, N, K)
    z = labels[:, :, None] == np.arange(1, K + 1)[None, None, :]
    w = (pos * pcw + neg * ncw) / nb                                           # [B,N]; 0 on an ignored anchor
    s = np.where(z, -x, x)
    ce, m, om = softplus_sigmoid(s)
    mod = np.ones_like(m) if gamma == 0.0 else m ** gamma
    alpha_t = np.where(z, alpha_pos, alpha_neg)
    cared = (pos | neg)[:, :, None] & np.ones((1, 1, K), bool)
    term = np.where(cared, mod * alpha_t * ce * w[:, :, None], 0.0)
    cls_sum = term.sum()
    if K == 1:
        cls_pos, cls_neg = term[pos].sum(), term[neg].sum()
    else:
        cls_pos, cls_neg = term[..., 1:].sum(), term[..., 0].sum()
    g = (cls_weight / B) * alpha_t * w[:, :, None] * mod * (gamma * om * ce + m)
    g = np.where(cared, np.where(z, -g, g), 0.0)
    grad[:, :, off_cls:off_cls + A * K] = g.reshape(B, H * W, A * K)
    structural[:, :, off_cls:off_cls + A * K] = ~cared.reshape(B, H * W, A * K)

    # localisation and direction: positives only
    bi, ni = np.nonzero(pos)
    cell, a = ni // A, ni % A
    nbp = nb[bi, 0]
    pred = np.stack([cells[bi, cell, off_box + a * 7 + j] for j in range(7)], 1).astype(np.float64)
    tgt = reg_targets[bi, ni].astype(np.float64)
    d = cw[None, :] * (pred - tgt)
    chain = np.ones_like(d)
    if len(bi):
        sp, cp, st, ct = np.sin(pred[:, 6]), np.cos(pred[:, 6]), np.sin(tgt[:, 6]), np.cos(tgt[:, 6])
        d[:, 6] = cw[6] * (sp * ct - cp * st)
        chain[:, 6] = cp * ct + sp * st                                        # cos(pred - tgt)
    ad = np.abs(d)
    quad = ad <= 1.0 / (sigma * sigma)
    loc_terms = np.where(quad, 0.5 * (ad * sigma) ** 2, ad - 0.5 / (sigma * sigma)) / nbp[:, None]
    loc_sum = loc_terms.sum()
    gl = (loc_weight / B) * cw[None, :] * np.where(quad, sigma * sigma * d, np.sign(d)) * chain / nbp[:, None]
    for j in range(7):
        grad[bi, cell, off_box + a * 7 + j] = gl[:, j]
        structural[bi, cell, off_box + a * 7 + j] = False
    dir_sum = 0.0
    if has_dir:
        rot = reg_targets[bi, ni, 6].astype(np.float32) + anchors[ni, 6].astype(np.float32)      # the fp32 sum
        t = (rot > 0).astype(np.int64)
        xt = cells[bi, cell, off_dir + a * 2 + t].astype(np.float64)
        xo = cells[bi, cell, off_dir + a * 2 + 1 - t].astype(np.float64)
        sp_, m_, _ = softplus_sigmoid(xo - xt)
        dir_sum = (sp_ / nbp).sum()
        gd = (dir_weight / B) * m_ / nbp
        grad[bi, cell, off_dir + a * 2 + 1 - t] = gd
        grad[bi, cell, off_dir + a * 2 + t] = -gd
        structural[bi, cell, off_dir + a * 2] = False
        structural[bi, cell, off_dir + a * 2 + 1] = False

    loc, cls = loc_weight * loc_sum / B, cls_weight * cls_sum / B
    dirl = dir_weight * dir_sum / B if has_dir else 0.0
    parts = np.array([loc, cls, dirl, cls_pos / B / pcw, cls_neg / B / ncw], np.float64)
    out = dict(parts=parts, num_pos=num_pos, total=np.float64((loc + cls) + dirl))
    if with_grad:
        out["grad"] = grad.reshape(B, H, W, C)
        out["structural"] = structural.reshape(B, H, W, C)
    return out


# ---------------------------------------------------------------------------------------------------- comparison
def compare_grad(got, want):
    """got fp32 [B,H,W,C] against the contract's result -> (elements outside the structural zeros, of those how many differ at all from
    the contract's float64 rounded to fp32, the worst distance in ulp, structural zeros whose bits are not +0.0, NaNs)"""
    got = np.ascontiguousarray(got, np.float32)
    st = want["structural"]
    apart = ulps_apart(got[~st], want["grad"][~st].astype(np.float32))
    return (int((~st).sum()), int((apart > 0).sum()), int(apart.max()) if apart.size else 0, int((got.view(np.int32)[st] != 0).sum()),
            int(np.isnan(got).sum()))
