"""What the two operators of include/minddet_hip_convbwd.h compute, restated in numpy float64: the weight gradient of a k x k / stride 1 /
same-padding convolution in a pack's column order with its block mask (md_conv_bwd_weight) and the data gradient of a pointwise
convolution through a ReLU mask (md_conv1x1_bwd_data).  The judges of tests/test_convbwd_ops_cpu.py (which pins them to torch-CPU
float64 autograd of F.conv2d), tests/test_convbwd_gpu.py and tests/test_cn_head_train_gpu.py; nothing here is tuned to a device.
The slab size, the chain length L(P) and the Gaussian bound of the weight gradient are those of tests/train_contract.py."""
import numpy as np

from tests import train_contract as tc

chain_length = tc.chain_length          # L(P): the same S, n and L as md_conv1x1_bwd_weight
wgrad_bound = tc.wgrad_bound


def columns(kernel, cin, korder):
    """[kernel^2, cin] int: col(t, i) of the header"""
    t, i = np.meshgrid(np.arange(kernel * kernel), np.arange(cin), indexing="ij")
    if korder == 0:
        return t * cin + i
    assert korder == 1 and cin % 64 == 0
    return (i // 64) * (kernel * kernel * 64) + t * 64 + i % 64


def shifted(X, kernel):
    """X [N,H,W,C] -> [kernel^2, N,H,W,C]: tap t = kernel ky + kx holds X[n, h + ky - pad, w + kx - pad], zero outside the image"""
    N, H, W, C = X.shape
    pad = (kernel - 1) // 2
    Z = np.zeros((N, H + 2 * pad, W + 2 * pad, C), X.dtype)
    Z[:, pad:pad + H, pad:pad + W] = X
    return np.stack([Z[:, ky:ky + H, kx:kx + W] for ky in range(kernel) for kx in range(kernel)])


def wgrad_kxk(x, dy, cin, cout, kernel=1, korder=0, x_c_off=0, dy_c_off=0, blocks=(), rows=None, kpad=None):
    """x [N,H,W,Cx] (the fp32 values of bf16 numbers), dy [N,H,W,Cy] f32 -> dict(dw [rows,kpad] f64, db [rows] f64, absdw, absdb: the
    sums of |dy x| and |dy| the bounds are stated in, live [rows,kpad] bool: the elements inside the layer and its blocks); rows / kpad
    default to cout / kernel^2 cin; everything outside `live` is 0.  blocks: (row0, rows, col0, cols); none = dense."""
    taps = kernel * kernel
    rows, kpad = cout if rows is None else rows, taps * cin if kpad is None else kpad
    X = shifted(np.asarray(x, np.float64)[..., x_c_off:x_c_off + cin], kernel).reshape(taps, -1, cin)
    D = np.asarray(dy, np.float64).reshape(-1, dy.shape[-1])[:, dy_c_off:dy_c_off + cout]
    mask = np.ones((cout, cin), bool)
    if len(blocks):
        mask[:] = False
        for r0, nr, c0, nc in blocks:
            mask[r0:r0 + nr, c0:c0 + nc] = True
    col = columns(kernel, cin, korder)
    out = dict(dw=np.zeros((rows, kpad)), db=np.zeros(rows), absdw=np.zeros((rows, kpad)), absdb=np.zeros(rows), live=np.zeros((rows, kpad), bool))
    for t in range(taps):
        out["dw"][:cout, col[t]] = (D.T @ X[t]) * mask
        out["absdw"][:cout, col[t]] = (np.abs(D).T @ np.abs(X[t])) * mask
        out["live"][:cout, col[t]] = mask
    out["db"][:cout] = D.sum(0)
    out["absdb"][:cout] = np.abs(D).sum(0)
    return out


def dgrad_chain_length(cout):
    """Ld(cout) of the header: one fp32 rounding per product of the fma chain over o"""
    return cout


def dgrad_1x1(dy, w, cin, cout, act=None, dy_c_off=0, act_c_off=0):
    """dy [N,H,W,Cy] f32, w [rows,kpad] (the fp32 values of the bf16 pack), act [N,H,W,Ca] (fp32 values of bf16 numbers) or None ->
    dict(dx [N,H,W,cin] f64, absdx: sum_o |dy w|, keep [N,H,W,cin] bool: act > 0).  Masked elements are 0 in dx and absdx."""
    D = np.asarray(dy, np.float64)[..., dy_c_off:dy_c_off + cout]
    Wm = np.asarray(w, np.float64)[:cout, :cin]
    dx, absdx = D @ Wm, np.abs(D) @ np.abs(Wm)
    keep = np.ones(dx.shape, bool)
    if act is not None:
        with np.errstate(invalid="ignore"):
            keep = np.asarray(act, np.float32)[..., act_c_off:act_c_off + cin] > 0        # false for -0, negatives and NaN
    return dict(dx=np.where(keep, dx, 0.0), absdx=np.where(keep, absdx, 0.0), keep=keep)


def dgrad_bound(cout, absdx):
    return dgrad_chain_length(cout) * 2.0 ** -24 * absdx
