"""GPU: md_grad_sumsq and md_adam_step (include/minddet_hip_train.h) against tests/train_contract.py on the tensors read back.

Conditions, fixed beforehand (as in the loss tests):
  md_grad_sumsq  within 2 float64 ulp sqrt(n) of the contract's sum (the order is fixed, another one than numpy's), bit-identical across calls
  md_adam_step   m, v and param within 1 fp32 ulp of the contract with at most 1 element in 10^4 differing (never more than 0 below 10^4
                 elements); exact zeros stay +0.0; shadow equals the bf16 rounding (nearest even) of the device's own new param bit for
                 bit; elements of a wider shadow tensor from ns on are untouched; bit-identical across calls."""
import numpy as np
import pytest
import torch

from tests import train_contract as tc
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
HYPER = dict(lr=1e-3, beta2=0.999, eps=1e-8)


@pytest.mark.parametrize("n", [1, 63, 64 * 1024 + 5])
def test_grad_sumsq_equals_the_contract(n):
    from minddet_amd import det_ops

    g = np.random.default_rng(n).normal(0, 3, n).astype(np.float32)
    gd = torch.from_numpy(g).to(DEV)
    got = [float(det_ops.grad_sumsq(gd, workspace=ws).cpu()[0]) for ws in (True, True, False)]
    want = tc.sumsq(g)
    print(f"grad_sumsq[n {n}]: device {got[0]!r}, contract {want!r}, {abs(got[0] - want) / np.spacing(want):.1f} ulp apart")
    assert abs(got[0] - want) <= 2 * np.spacing(want) * np.sqrt(n)
    assert got[0] == got[1] == got[2]                                                    # across calls and scratch forms, bit for bit


def _state_after_three_steps(rng, n):
    """param, m, v (fp32) after three contract steps from zero moments: the state a fourth step meets"""
    f32 = lambda a: np.asarray(a, np.float32)
    p, m, v = f32(rng.normal(0, 0.1, n)), np.zeros(n, np.float32), np.zeros(n, np.float32)
    b1p, b2p = np.float32(1), np.float32(1)
    for _ in range(3):
        b1p, b2p = np.float32(b1p * np.float32(0.9)), np.float32(b2p * np.float32(0.999))
        p, m, v = tc.adam(f32(rng.normal(0, 1, n)), p, m, v, beta1=0.9, beta1_power=float(b1p), beta2_power=float(b2p), weight_decay=1e-4, **HYPER)
    return p, m, v, float(np.float32(b1p * np.float32(0.9))), float(np.float32(b2p * np.float32(0.999)))


def _step(g, p, m, v, ns, shadow_len, offset=0, **kw):
    """one md_adam_step on copies -> (param, m, v, shadow bits or None) numpy; offset: the tensors are views at that element of larger
    ones (an unaligned base pointer)"""
    from minddet_amd import det_ops

    def dev(a):
        t = torch.zeros(len(a) + offset, dtype=torch.float32, device=DEV)
        t[offset:] = torch.from_numpy(a)
        return t[offset:]

    gd, pd, md, vd = dev(g), dev(p), dev(m), dev(v)
    whole = torch.full((shadow_len + offset,), 0x7FC1, dtype=torch.int16, device=DEV).view(torch.bfloat16) if shadow_len is not None else None
    sh = None if whole is None else whole[offset:offset + ns]
    sumsq = kw.pop("sumsq", None)
    sd = None if sumsq is None else torch.tensor(list(sumsq), dtype=torch.float64, device=DEV)
    det_ops.adam_step(gd, pd, md, vd, sumsq=sd, shadow=sh if (sh is not None and ns > 0) else None, **kw)
    torch.cuda.synchronize()
    bits = None if whole is None else whole.view(torch.int16).cpu().numpy().view(np.uint16)[offset:]
    return pd.cpu().numpy(), md.cpu().numpy(), vd.cpu().numpy(), bits


def _hold(got, args, n, **kw):
    """the device's (param, m, v) against the contract on `args` = (grad, param, m, v): within 1 ulp, at most 1 in 10^4 differing; a value
    that is exactly zero before rounding is +0.0 on the device (one that underflows keeps its sign, as the contract's rounding does)"""
    want, exact = tc.adam(*args, **kw), tc.adam(*args, rounded=False, **kw)
    for name, a, b, e in zip(("param", "m", "v"), got[:3], want, exact):
        assert not np.isnan(a).any() and not np.isnan(b).any(), name
        apart = tc.ulps_apart(a, b)
        ndiff, worst = int((apart > 0).sum()), int(apart.max())
        print(f"adam[{name}, n {n}]: {ndiff} of {n} differ, worst {worst} ulp")
        assert worst <= 1 and ndiff * 10000 <= n, (name, ndiff, worst)
        assert (a[e == 0].view(np.uint32) == 0).all(), name                              # exact zeros stay +0.0
        assert np.array_equal(np.signbit(a[b == 0]), np.signbit(b[b == 0])), name
    return want


@pytest.mark.parametrize("n,ns", [(1, 0), (1, 1), (7, 5), (7, 7), (4096 + 3, 0), (4096 + 3, 5), (4096 + 3, 4096 + 3)])
@pytest.mark.parametrize("clip", ["active", "inactive", "none"])
def test_adam_step_equals_the_contract(n, ns, clip):
    rng = np.random.default_rng([n, ns])
    p, m, v, b1p, b2p = _state_after_three_steps(rng, n)
    g = rng.normal(0, 1, n).astype(np.float32)
    assert tc.sumsq(g) < 100.0 ** 2
    ss = None if clip == "none" else [tc.sumsq(g), 100.0 ** 2 - tc.sumsq(g)]             # K = 2: the second range carries the norm to 100
    max_norm = None if clip == "none" else (35.0 if clip == "active" else 1000.0)
    if ss is not None:
        total = np.sqrt(ss[0] + ss[1])
        assert abs(total - 100.0) < 1e-6 and (max_norm / (total + 1e-6) < 1) == (clip == "active")
    kw = dict(beta1=0.9, beta1_power=b1p, beta2_power=b2p, weight_decay=1e-4, grad_scale=1.0 / 512 if clip == "inactive" else 1.0, max_norm=max_norm, **HYPER)
    got = _step(g, p, m, v, ns, shadow_len=n + 3, sumsq=ss, **kw)
    _hold(got, (g, p, m, v), n, sumsq=ss, **kw)
    assert np.array_equal(got[3][:ns], tc.bf16_bits(got[0][:ns]))                         # bf16 of the device's own new param
    assert (got[3][ns:] == 0x7FC1).all()                                                 # the rest of a wider shadow tensor is untouched
    again = _step(g, p, m, v, ns, shadow_len=n + 3, sumsq=ss, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_adam_step_on_an_unaligned_base_pointer():
    n, ns = 4096 + 3, 4096 + 3
    rng = np.random.default_rng(5)
    p, m, v, b1p, b2p = _state_after_three_steps(rng, n)
    g = rng.normal(0, 1, n).astype(np.float32)
    kw = dict(beta1=0.9, beta1_power=b1p, beta2_power=b2p, weight_decay=1e-4, **HYPER)
    got = _step(g, p, m, v, ns, shadow_len=n + 3, offset=1, **kw)                         # every tensor a view at element 1
    _hold(got, (g, p, m, v), n, **kw)
    assert np.array_equal(got[3][:ns], tc.bf16_bits(got[0][:ns])) and (got[3][ns:] == 0x7FC1).all()
    aligned = _step(g, p, m, v, ns, shadow_len=n + 3, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, aligned))                  # the scalar and the 16-byte path agree bit for bit


def test_adam_step_on_extreme_gradients_gives_no_nan():
    g = np.array([0.0, -0.0, 1e-30, -1e-30, 1e30, -1e30, 1.0, 0.0, -0.0], np.float32)
    n = len(g)
    p = np.linspace(-1, 1, n).astype(np.float32)
    p[7:] = 0.0
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    kw = dict(beta1=0.9, beta1_power=0.9, beta2_power=0.999, **HYPER)
    for ss, mn in (([tc.sumsq(g)], 35.0), (None, None)):
        got = _step(g, p, m, v, n, shadow_len=n, sumsq=ss, max_norm=mn, **kw)
        want = _hold(got, (g, p, m, v), n, sumsq=ss, max_norm=mn, **kw)                   # (NaN nowhere is part of it)
        assert np.array_equal(got[0][[0, 1]], p[[0, 1]])                                  # a zero gradient on zero state: the update is exactly 0
        assert (got[0][7:].view(np.uint32) == 0).all() and (got[1][[0, 1, 7, 8]].view(np.uint32) == 0).all() and (got[2][[0, 1, 7, 8]].view(np.uint32) == 0).all()
    # the state the huge gradient leaves (v = inf in fp32) takes another step without a NaN
    assert np.isinf(want[2]).any()
    got2 = _step(g, *want, n, shadow_len=n, beta1=0.9, beta1_power=0.81, beta2_power=0.998, **HYPER)
    _hold(got2, (g,) + tuple(want), n, beta1=0.9, beta1_power=0.81, beta2_power=0.998, **HYPER)
