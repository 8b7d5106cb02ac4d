"""What the two operators of include/minddet_hip_groupedbwd.h compute, restated in numpy float64: the data gradient of md_conv2d_grouped
through a ReLU mask (md_conv2d_grouped_bwd_data) and the weight and bias gradient of every group in the grouped pack's layout
(md_conv2d_grouped_bwd_weight).  The judges of tests/test_groupedbwd_ops_cpu.py (which pins them to torch-CPU float64 autograd of
F.conv2d(..., groups=G)), tests/test_groupedbwd_gpu.py and tests/test_cp_head_train_gpu.py; nothing here is tuned to a device.
A table is the forward call's: dict(k, x_c_off, cout [G], y_off [G], w_row [G]).  The slab size, the chain length L(P) and the Gaussian
bound of the weight gradient are those of tests/train_contract.py."""
import numpy as np

from tests import train_contract as tc
from tests.convbwd_contract import shifted

chain_length = tc.chain_length          # L(P): the same S, n and L as md_conv_bwd_weight
wgrad_bound = tc.wgrad_bound


def table(k, couts, y_offs=None, w_rows=None, x_c_off=0):
    couts = [int(c) for c in couts]
    side = [sum(couts[:g]) for g in range(len(couts))]
    return dict(k=int(k), x_c_off=int(x_c_off), cout=couts, y_off=list(side if y_offs is None else y_offs), w_row=list(side if w_rows is None else w_rows))


def dgrad_chain_length(k, cout):
    """Ld(k, cout) of the header: one fp32 rounding per product of the fma chain over (t, o)"""
    return k * k * cout


def dgrad_grouped(dy, w, tb, act=None, cdx=None):
    """dy [N,H,W,Cy] f32, w [R, k k 64] (the fp32 values of the bf16 pack), act [N,H,W,Ca] (fp32 values of bf16 numbers) or None ->
    dict(dx [N,H,W,cdx] f64, absdx: sum |dy w|, keep bool: act > 0, covered bool [cdx]: the channels some group writes, ld [cdx]: the
    chain length of the channel's group).  Masked and uncovered elements are 0 in dx and absdx."""
    k, G = tb["k"], len(tb["cout"])
    cdx = tb["x_c_off"] + 64 * G if cdx is None else cdx
    D = np.asarray(dy, np.float64)
    Wm = np.asarray(w, np.float64)
    N, H, Wd, _ = D.shape
    dx, absdx = np.zeros((N, H, Wd, cdx)), np.zeros((N, H, Wd, cdx))
    covered, ld = np.zeros(cdx, bool), np.zeros(cdx)
    for g in range(G):
        co, yo, wr, c0 = tb["cout"][g], tb["y_off"][g], tb["w_row"][g], tb["x_c_off"] + 64 * g
        # dx[q] = sum_t dy[q - d_t] w_t: tap t of `shifted` holds X[q + d_t], so the term of tap t is tap (k k - 1 - t) of shifted(dy)
        S = shifted(D[..., yo:yo + co], k)
        A = shifted(np.abs(D[..., yo:yo + co]), k)
        for t in range(k * k):
            Wt = Wm[wr:wr + co, t * 64:(t + 1) * 64]
            dx[..., c0:c0 + 64] += S[k * k - 1 - t] @ Wt
            absdx[..., c0:c0 + 64] += A[k * k - 1 - t] @ np.abs(Wt)
        covered[c0:c0 + 64] = True
        ld[c0:c0 + 64] = dgrad_chain_length(k, co)
    keep = np.ones(dx.shape, bool)
    if act is not None:
        with np.errstate(invalid="ignore"):
            keep = np.asarray(act, np.float32)[..., :cdx] > 0                              # false for -0, negatives and NaN
    keep = keep & covered
    return dict(dx=np.where(keep, dx, 0.0), absdx=np.where(keep, absdx, 0.0), keep=keep, covered=covered, ld=ld)


def dgrad_bound(res):
    return res["ld"] * 2.0 ** -24 * res["absdx"]


def wgrad_grouped(x, dy, tb, rows):
    """x [N,H,W,C] (the fp32 values of bf16 numbers), dy [N,H,W,Cy] f32 -> dict(dw [rows, k k 64] f64, db [rows] f64, absdw, absdb: the
    sums of |dy x| and |dy| the bounds are stated in, live [rows] bool: the rows some group owns); every other row is 0."""
    k, G = tb["k"], len(tb["cout"])
    taps = k * k
    out = dict(dw=np.zeros((rows, taps * 64)), db=np.zeros(rows), absdw=np.zeros((rows, taps * 64)), absdb=np.zeros(rows), live=np.zeros(rows, bool))
    Dall = np.asarray(dy, np.float64).reshape(-1, dy.shape[-1])
    for g in range(G):
        co, yo, wr, c0 = tb["cout"][g], tb["y_off"][g], tb["w_row"][g], tb["x_c_off"] + 64 * g
        X = shifted(np.asarray(x, np.float64)[..., c0:c0 + 64], k).reshape(taps, -1, 64)
        D = Dall[:, yo:yo + co]
        for t in range(taps):
            out["dw"][wr:wr + co, t * 64:(t + 1) * 64] = D.T @ X[t]
            out["absdw"][wr:wr + co, t * 64:(t + 1) * 64] = np.abs(D).T @ np.abs(X[t])
        out["db"][wr:wr + co] = D.sum(0)
        out["absdb"][wr:wr + co] = np.abs(D).sum(0)
        out["live"][wr:wr + co] = True
    return out
