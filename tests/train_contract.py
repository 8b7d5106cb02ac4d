"""What the training-step operators of include/minddet_hip_train.h compute, restated in numpy float64: the weight gradient of a pointwise
convolution (md_conv1x1_bwd_weight), the squared norm (md_grad_sumsq) and the reference's Adam step (md_adam_step:
centerpoint/det3d_ms/solver/custom_adam.py:590-668 around the dense update of :188-222).  The judges of tests/test_train_ops_cpu.py,
tests/test_conv_bwd_gpu.py, tests/test_optim_gpu.py and tests/test_pp_head_train_gpu.py; nothing here is tuned to a device."""
import numpy as np

SLAB_MIN, MAX_SLABS, SUM_WAYS = 256, 256, 8      # MD_CONV1X1_BWD_SLAB_MIN / _MAX_SLABS / _SUM_WAYS (the CPU test reads them from the header)


def bf16_round(x):
    """fp32 -> the fp32 value of its bf16 rounding, round to nearest even (finite values)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def bf16_bits(x):
    """fp32 -> uint16 bits of its bf16 rounding"""
    return (bf16_round(x).view(np.uint32) >> 16).astype(np.uint16)


def wgrad(x, dy, cin, cout, x_c_off=0, dy_c_off=0, rows=None, kpad=None):
    """x [N,H,W,Cx] (the fp32 values of bf16 numbers), dy [N,H,W,Cy] f32 -> dict(dw [rows,kpad] f64, db [rows] f64, absdw, absdb: the
    sums of |dy x| and |dy| the error bounds are stated in); rows / kpad default to cout / cin; padding is 0"""
    rows, kpad = cout if rows is None else rows, cin if kpad is None else kpad
    X = np.asarray(x, np.float64).reshape(-1, x.shape[-1])[:, x_c_off:x_c_off + cin]
    D = np.asarray(dy, np.float64).reshape(-1, dy.shape[-1])[:, dy_c_off:dy_c_off + cout]
    out = dict(dw=np.zeros((rows, kpad)), db=np.zeros(rows), absdw=np.zeros((rows, kpad)), absdb=np.zeros(rows))
    out["dw"][:cout, :cin] = D.T @ X
    out["absdw"][:cout, :cin] = np.abs(D).T @ np.abs(X)
    out["db"][:cout] = D.sum(0)
    out["absdb"][:cout] = np.abs(D).sum(0)
    return out


def slab_pixels(P):
    """S of the header: pixels per slab of the first launch"""
    per = -(-P // MAX_SLABS)
    return max(SLAB_MIN, -(-per // 16) * 16)


def chain_length(P):
    """L(P) of the header: the longest chain of fp32 roundings behind an element of dw or db"""
    S = slab_pixels(P)
    n = -(-P // S)
    return S // 4 + 3 + -(-n // SUM_WAYS) + (SUM_WAYS - 1)


def wgrad_bound(P, absdw):
    """the Gaussian-data condition: |dw - dw64| <= (2^-16 + L 2^-24) sum_p |dy x|"""
    return (2.0 ** -16 + chain_length(P) * 2.0 ** -24) * absdw


def sumsq(grad):
    """float64 sum of squares of the fp32 values"""
    g = np.asarray(grad, np.float32).astype(np.float64)
    return float(np.sum(g * g))


def adam(grad, param, m, v, *, lr, beta1, beta2, beta1_power, beta2_power, eps=1e-8, weight_decay=0.0, sumsq=None, max_norm=None,
         grad_scale=1.0, rounded=True):
    """Adam.construct for one flat range: every term float64 from the fp32 operands, in the header's order.
    sumsq: iterable of float64 squared norms (None: no clip) -> (param', m', v'), each rounded once to fp32 (rounded=False: float64)"""
    g = np.asarray(grad, np.float32).astype(np.float64)
    p = np.asarray(param, np.float32).astype(np.float64)
    m = np.asarray(m, np.float32).astype(np.float64)
    v = np.asarray(v, np.float32).astype(np.float64)
    if sumsq is not None:
        t = np.float64(0.0)
        for s in np.asarray(sumsq, np.float64).reshape(-1):
            t = t + s
        coef = np.float64(max_norm) / (np.sqrt(t) + np.float64(1e-6))
        if coef < 1:
            g = g * coef
    g = g + np.float64(weight_decay) * p
    g = g * np.float64(grad_scale)
    b1, b2 = np.float64(beta1), np.float64(beta2)
    with np.errstate(over="ignore", invalid="ignore"):
        m2 = b1 * m + (1.0 - b1) * g
        v2 = b2 * v + (1.0 - b2) * (g * g)
        lr_t = np.float64(lr) * np.sqrt(1.0 - np.float64(beta2_power)) / (1.0 - np.float64(beta1_power))
        p2 = p - lr_t * (m2 / (np.sqrt(v2) + np.float64(eps)))
        if not rounded:
            return p2, m2, v2
        return p2.astype(np.float32), m2.astype(np.float32), v2.astype(np.float32)


def ulps_apart(a, b):
    """fp32 arrays -> the distance in representable values (0 for equal values, +0 and -0 included)"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
