"""The contract of md_cp_loss / md_cp_loss_grad (include/minddet_hip_cploss.h) in numpy float64: per task the clipped probability, slot
validity, num_pos, the focal terms, box_loss / loc_loss, total, and the analytic gradient of total with respect to every head element.
Inputs are the values the operator is given (the bf16 logits widened exactly, the fp32 targets); nothing here is rounded.
tests/test_cp_loss_cpu.py compares it with a literal torch-float64 transcription of the reference's loss under autograd;
tests/test_cp_loss_gpu.py holds the device result to it.  The comparison helpers both tests use live here too."""
import numpy as np

LO, HI = 1e-4, 1 - 1e-4


def columns(off):
    """one task's {head: first channel} -> (head channel, anno_box column) of each box_loss column: anno_box is (reg 2, height, dim 3,
    vel 2, rot 2) while the head stores rot before vel; without vel the rot channels meet target columns 8, 9 as box_loss columns 6, 7"""
    chans = [off["reg"], off["reg"] + 1, off["height"], off["dim"], off["dim"] + 1, off["dim"] + 2]
    if "vel" in off and off["vel"] >= 0:
        return np.array(chans + [off["vel"], off["vel"] + 1, off["rot"], off["rot"] + 1]), np.arange(10)
    return np.array(chans + [off["rot"], off["rot"] + 1]), np.array([0, 1, 2, 3, 4, 5, 8, 9])


def loss(head, hm, anno_box, ind, mask, cat, *, task_offsets, num_classes, weight, code_weights, with_grad=True):
    """head [B,H,W,Cp] (float array of the bf16 values; channels no head owns may hold anything), hm [B,T,C,H,W], anno_box [B,T,M,10],
    ind / mask / cat [B,T,M] -> dict of float64: parts [T,12], num_pos [T], total (scalar) and grad [B,H,W,Cp]"""
    B, H, W, Cp = head.shape
    HW, T = H * W, len(num_classes)
    cw = np.zeros(10)
    cw[:len(code_weights)] = np.asarray(code_weights, np.float64)
    weight = float(weight)
    flat = head.reshape(B, HW, Cp)
    grad = np.zeros((B, HW, Cp))
    parts, num_pos, total = np.zeros((T, 12)), np.zeros(T), 0.0
    for t, (off, nc) in enumerate(zip(task_offsets, num_classes)):
        x = flat[:, :, off["hm"]:off["hm"] + nc].astype(np.float64)
        with np.errstate(over="ignore"):
            s = 1.0 / (1.0 + np.exp(-x))
        is_open = (s > LO) & (s < HI)                                          # the clip passes the gradient
        p = np.clip(s, LO, HI)
        target = hm[:, t, :nc].astype(np.float64).reshape(B, nc, HW).transpose(0, 2, 1)
        g4 = (1.0 - target) ** 4
        l1p = np.log(1.0 - p)
        neg = (l1p * p ** 2 * g4).sum()
        ghm = np.where(is_open, g4 * p ** 2 * (2.0 * (1.0 - p) * l1p - p), 0.0)

        i_t, c_t = ind[:, t].astype(np.int64), cat[:, t].astype(np.int64)
        valid = (mask[:, t] != 0) & (i_t >= 0) & (i_t < HW) & (c_t >= 0) & (c_t < nc)
        b, k = np.nonzero(valid)
        i, c = i_t[b, k], c_t[b, k]
        n = len(b)
        ps = p[b, i, c]
        pos = (np.log(ps) * (1.0 - ps) ** 2).sum()
        np.add.at(ghm, (b, i, c), np.where(is_open[b, i, c], (1.0 - ps) ** 2 * ((1.0 - ps) - 2.0 * ps * np.log(ps)), 0.0))
        hm_loss = -neg if n == 0 else -(pos + neg) / n
        grad[:, :, off["hm"]:off["hm"] + nc] = (-1.0 if n == 0 else -1.0 / n) * ghm

        chans, tcols = columns(off)
        d = flat[b, i][:, chans].astype(np.float64) - anno_box[b, t, k][:, tcols].astype(np.float64)
        box = np.zeros(10)
        box[:len(chans)] = np.abs(d).sum(0) / (n + 1e-4)
        loc = (box * cw).sum()
        np.add.at(grad, (b[:, None], i[:, None], chans[None, :]), weight * cw[:len(chans)] * np.sign(d) / (n + 1e-4))
        parts[t, 0], parts[t, 1], parts[t, 2:] = hm_loss, loc, box
        num_pos[t] = n
        total += hm_loss + weight * loc
    out = dict(parts=parts, num_pos=num_pos, total=np.float64(total))
    if with_grad:
        out["grad"] = grad.reshape(B, H, W, Cp)
    return out


# ---------------------------------------------------------------------------------------------------- comparison
def ulps_apart(a, b):
    """fp32 arrays -> how many representable values apart (signed values; -0 and +0 coincide)"""
    def ordered(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def compare_losses(got, want):
    """parts / num_pos / total of a result (fp32) against the contract's float64 rounded to fp32 -> the worst distance in ulp"""
    worst = 0
    for k in ("parts", "num_pos", "total"):
        g = np.asarray(got[k], np.float32).reshape(-1)
        w = np.asarray(want[k], np.float64).astype(np.float32).reshape(-1)
        assert g.shape == w.shape and np.isfinite(g).all(), k
        worst = max(worst, int(ulps_apart(g, w).max()))
    return worst


def compare_grad(got, want64):
    """-> (elements that are non-zero in the contract, of those how many differ at all, the worst distance in ulp, wrong zeros,
    NaNs): got fp32 against the contract's float64 rounded to fp32"""
    got = np.asarray(got, np.float32)
    zero = want64 == 0.0
    apart = ulps_apart(got[~zero], want64[~zero].astype(np.float32))
    return (int((~zero).sum()), int((apart > 0).sum()), int(apart.max()) if apart.size else 0, int((got[zero] != 0).sum()),
            int(np.isnan(got).sum()))
