"""The contract of md_cn_loss / md_cn_loss_grad (include/minddet_hip_cn.h) in numpy float64: the clipped probability, num_pos, the two
focal sums, slot validity, wh_loss / off_loss, total, and the analytic gradient of total with respect to every head element.  Inputs are
the values the operator is given (the bf16 logits widened exactly, the fp32 targets); nothing here is rounded.
tests/test_cn_loss_cpu.py compares it with a literal torch-float64 transcription of the reference's loss under autograd;
tests/test_cn_loss_gpu.py holds the device result to it.  The comparison helpers are those of tests/cp_loss_contract.py."""
import numpy as np

from tests.cp_loss_contract import compare_grad, compare_losses, ulps_apart  # noqa: F401

LO, HI = 1e-4, 1 - 1e-4


def loss(head, hm, ind, reg_mask, wh, reg, *, num_classes, off_hm, off_wh, off_reg, hm_weight, wh_weight, off_weight, with_grad=True):
    """head [B,H,W,Cp] (float array of the bf16 values; channels no head owns may hold anything), hm [B,C,H,W], ind / reg_mask [B,M],
    wh / reg [B,M,2] -> dict of float64: parts [3] (hm_loss, wh_loss, off_loss), num_pos [1], total (scalar) and grad [B,H,W,Cp]"""
    B, H, W, Cp = head.shape
    HW, C = H * W, int(num_classes)
    hm_weight, wh_weight, off_weight = float(hm_weight), float(wh_weight), float(off_weight)
    flat = head.reshape(B, HW, Cp)
    grad = np.zeros((B, HW, Cp))

    x = flat[:, :, off_hm:off_hm + C].astype(np.float64)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-x))
    is_open = (s > LO) & (s < HI)                                              # the clip passes the gradient
    p = np.clip(s, LO, HI)
    om = 1.0 - p
    target = hm.astype(np.float64).reshape(B, C, HW).transpose(0, 2, 1)
    with np.errstate(invalid="ignore"):
        is_pos, is_neg = target == 1.0, target < 1.0                           # hm > 1 or NaN: in neither sum
    num_pos = float(is_pos.sum())
    n = 1.0 if num_pos == 0 else num_pos
    lp, l1p = np.log(p), np.log(om)
    q = np.where(is_neg, 1.0 - target, 0.0)
    g4 = (q * q) * (q * q)
    pos = np.where(is_pos, lp * (om * om), 0.0).sum()
    neg = np.where(is_neg, l1p * (p * p) * g4, 0.0).sum()
    hm_loss = -(pos + neg) / n
    d = np.where(is_pos, (om * om) * (om - 2.0 * p * lp), np.where(is_neg, g4 * (p * p) * (2.0 * om * l1p - p), 0.0))
    grad[:, :, off_hm:off_hm + C] = np.where(is_open, (-hm_weight / n) * d, 0.0) + 0.0      # (+ 0.0: -0.0, as hm_weight 0 gives, becomes +0.0)

    i_all = ind.astype(np.int64)
    valid = (reg_mask != 0) & (i_all >= 0) & (i_all < HW)
    b, k = np.nonzero(valid)
    i = i_all[b, k]
    den = 2.0 * len(b) + 1e-4
    use_off = off_reg != -1 and off_weight > 0
    losses = []
    for on, off, tgt, weight in ((True, off_wh, wh, wh_weight), (use_off, off_reg, reg, off_weight)):
        if not on:
            losses.append(0.0)
            continue
        diff = flat[b, i][:, off:off + 2].astype(np.float64) - tgt[b, k].astype(np.float64)
        losses.append(np.abs(diff).sum() / den)
        sgn = np.zeros((B, HW, 2), np.int64)
        np.add.at(sgn, (b, i), np.sign(diff).astype(np.int64))
        grad[:, :, off:off + 2] = np.where(sgn != 0, weight * sgn / den, 0.0)
    total = (hm_weight * hm_loss + wh_weight * losses[0]) + off_weight * losses[1]
    out = dict(parts=np.array([hm_loss, losses[0], losses[1]]), num_pos=np.array([num_pos]), total=np.float64(total))
    if with_grad:
        out["grad"] = grad.reshape(B, H, W, Cp)
    return out

