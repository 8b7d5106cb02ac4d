"""CPU: the training-step operators without a GPU -- the ABI of include/minddet_hip_train.h (the three operators and the workspace
functions exported, the semantic refusals answered before any device call, the ctypes mirrors laid out as
the header says), the contract tests/train_contract.py against a literal torch-float64 transcription of the reference's dense Adam
update with its global-norm clip (custom_adam.py:188-222, 590-600), optim.OneCycle against the reference's vectors bit for bit, and the
exclusion check that gives tests/test_conv_bwd_gpu.py its teeth: on the sixteen-bit inputs the exact result is an fp32 number and a dy
rounded once to bf16 misses it nearly everywhere.

Criterion of the Adam comparison, fixed beforehand: 1e-12 relative before rounding.  Measured: <= 4e-16."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from minddet_amd import _lib, det_ops, optim
from tests import train_cases, train_contract as tc
from tests import abi_header as ah
from tests.abi_cases import B16, U8
from tests.abi_cases_train import CASES, F64, AdamAttrs, Conv1x1Bwd
from tests.abi_derive import attr, both, lib_handle, raw, rc, refuse_single_defects, shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = ah.header("minddet_hip_train.h")
OPS = ["md_conv1x1_bwd_weight", "md_grad_sumsq", "md_adam_step"]


def _case(tag_part, sym):
    return next(c for c in CASES if c.sym == sym and tag_part in c.tag)


def test_header_declares_the_operators_and_the_library_exports_them():
    assert ah.aot_symbols(HDR) == OPS and '#include "minddet_hip.h"' in HDR
    ws = re.findall(r"^extern int64_t (\w+_workspace_bytes)\((?:int64_t \w+(?:, )?)+\);", HDR, flags=re.M)
    assert ws == ["md_conv1x1_bwd_weight_workspace_bytes", "md_grad_sumsq_workspace_bytes"]
    for fn in ws:                                      # each directly under its operator
        assert re.search(rf"^int {fn[:-len('_workspace_bytes')]}\(MD_AOT_ARGS\);\nextern int64_t {fn}\(", HDR, flags=re.M), fn
    assert "custom_adam.py:590-668" in HDR and "minddet_hip_train.h" in open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    assert {c.sym for c in CASES} == set(OPS) and len({c.id for c in CASES}) == len(CASES)
    lib = lib_handle()
    for sym in OPS:
        assert getattr(lib, sym)(0, None, None, None, None, None, None) == 1             # wrong parameter count, before anything else
    for sym in ws:
        assert hasattr(lib, sym)
    # one valid row per optional-operand form
    assert {c.tag for c in CASES if c.sym == OPS[0]} == {"[pool]", "[workspace]", "[pool, no db]", "[workspace, no db]"}
    assert {c.tag for c in CASES if c.sym == OPS[2]} == {"[sumsq, shadow]", "[sumsq, no shadow]", "[no sumsq, shadow]", "[no sumsq, no shadow]"}


def test_workspace_functions_follow_the_headers_formulas():
    defines = ah.defines(HDR)
    assert (defines["MD_CONV1X1_BWD_SLAB_MIN"], defines["MD_CONV1X1_BWD_MAX_SLABS"], defines["MD_CONV1X1_BWD_SUM_WAYS"]) == \
        (tc.SLAB_MIN, tc.MAX_SLABS, tc.SUM_WAYS)
    assert (defines["MD_CONV1X1_BWD_MAX_CIN"], defines["MD_CONV1X1_BWD_MAX_COUT"]) == (1024, 256)
    for P, cin, cout in ((1, 8, 1), (15, 8, 3), (256, 8, 16), (257, 8, 17), (2145, 384, 20), (4 * 248 * 216, 384, 24), (66048, 8, 1)):
        S = tc.slab_pixels(P)
        n, R = -(-P // S), -(-cout // 16) * 16
        assert n <= tc.MAX_SLABS and S % 16 == 0
        assert det_ops.conv1x1_bwd_weight_workspace_bytes(P, cin, cout) == 4 * n * R * (cin + 1), (P, cin, cout)
    assert tc.slab_pixels(4 * 248 * 216) == 848 and tc.chain_length(4 * 248 * 216) == 212 + 3 + 32 + 7
    assert tc.chain_length(70) == 64 + 3 + 1 + 7                                           # one slab of the minimum size
    assert "L(P) = S / 4 + 3 + ceil(n / 8) + 7" in HDR
    assert [det_ops.grad_sumsq_workspace_bytes(n) for n in (1, 4096, 4097, 4096 * 1024 + 1)] == [8, 8, 16, 8 * 1024]
    assert defines["MD_GRAD_SUMSQ_CHUNK"] == 4096 and defines["MD_GRAD_SUMSQ_MAX_BLOCKS"] == 1024
    lib = lib_handle()
    for fn, n in (("md_conv1x1_bwd_weight_workspace_bytes", 3), ("md_grad_sumsq_workspace_bytes", 1)):      # a negative extent answers -1
        f = getattr(lib, fn)
        f.restype, f.argtypes = C.c_int64, [C.c_int64] * n
        assert f(*[8] * n) > 0 and all(f(*[-1 if j == k else 8 for j in range(n)]) == -1 for k in range(n)), fn
    with pytest.raises(_lib.MindDetHipError):
        det_ops.conv1x1_bwd_weight_workspace_bytes(-1, 8, 1)
    with pytest.raises(_lib.MindDetHipError):
        det_ops.grad_sumsq_workspace_bytes(-1)


def test_ctypes_mirrors_have_the_headers_layout():
    conv = ah.struct_of("md_conv1x1_bwd_attrs", HDR)
    adam = ah.struct_of("md_adam_attrs", HDR)
    assert C.sizeof(conv) == 5 * 4 and C.sizeof(adam) == 10 * 8

    for got in (det_ops._Conv1x1BwdAttrs, Conv1x1Bwd):
        assert ah.same_layout(got, conv), got
    for got in (det_ops._AdamAttrs, AdamAttrs):
        assert ah.same_layout(got, adam), got
    at = det_ops.adam_attrs(1e-3, 0.9, 0.999, 0.81, 0.998, eps=1e-8, weight_decay=1e-4, max_norm=35.0, grad_scale=0.5)
    assert [getattr(at, n) for n, _ in at._fields_] == [1e-3, 0.9, 0.999, 0.81, 0.998, 1e-8, 1e-4, 35.0, 0.5, 0.0]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_train", case)


@pytest.mark.parametrize("tag", ["[pool]", "[workspace]"])
def test_conv_bwd_semantic_refusals_return_the_documented_codes(tag):
    ARG, SIZE = 2, 4
    case = _case(tag, "md_conv1x1_bwd_weight")
    edits = [
        attr("reserved0", 1), attr("reserved0", -1), attr("cin", 0), attr("cin", -8), attr("cout", 0), attr("cout", -1),
        attr("x_c_off", -8), attr("dy_c_off", -1),
        attr("x_c_off", 16), attr("cin", 24), attr("dy_c_off", 6), attr("cout", 7),            # a channel range outside x / dy
        shape(0, (0, 3, 5, 16), B16), shape(0, (1, 0, 5, 16), B16), shape(1, (1, 3, 0, 8)),     # no pixel
        shape(1, (1, 3, 4, 8)), shape(1, (2, 3, 5, 8)), shape(0, (1, 5, 3, 16), B16),           # x and dy over different pixels
        shape(2, (2, 64)), shape(2, (32, 7)), shape(3, (2,)),                                   # dw / db smaller than the layer
    ]
    for i, e in enumerate(edits):
        assert rc(case, e) == ARG, i
    for o, k in ((2, 0), (2, 1), (3, 0), (3, 1), (3, 2)):                                          # an output at another operand's address
        assert raw(case, same=[(o, k)]) == ARG, (o, k)
    # the stated limits: each edit keeps every extent consistent, so the limit alone refuses it
    wide_x = both(shape(0, (1, 3, 5, 24), B16), attr("x_c_off", 0))
    assert rc(case, both(wide_x, attr("cin", 12))) == SIZE
    many = both(shape(1, (1, 3, 5, 264)), shape(2, (264, 64)), shape(3, (264,)), attr("dy_c_off", 0))
    assert rc(case, both(many, attr("cout", 257))) == SIZE
    wide = both(shape(0, (1, 3, 5, 1040), B16), shape(2, (32, 1088)), attr("x_c_off", 0))
    assert rc(case, both(wide, attr("cin", 1032))) == SIZE
    huge = both(shape(0, (2 ** 16, 2 ** 15, 1, 16), B16), shape(1, (2 ** 16, 2 ** 15, 1, 8)))   # P = 2^31
    assert raw(case, huge) == SIZE
    assert raw(case, shape(0, (2 ** 16, 2 ** 15, 1, 16), B16)) == ARG                            # (dy no longer matches)
    if tag == "[workspace]":
        assert rc(case, shape(4, (575,), U8)) == SIZE                                            # one byte short of 4 x 16 x 9


@pytest.mark.parametrize("tag", ["[sumsq, shadow]", "[no sumsq, no shadow]"])
def test_adam_semantic_refusals_return_the_documented_codes(tag):
    ARG, SIZE = 2, 4
    case = _case(tag, "md_adam_step")
    clip, shadow = not case.operands[1].null, not case.operands[5].null
    nan, inf = float("nan"), float("inf")
    edits = [
        attr("reserved0", 1.0), attr("reserved0", -1e-300), attr("lr", -1e-3), attr("lr", nan), attr("lr", inf), attr("beta1", 1.0),
        attr("beta1", -0.1), attr("beta2", 1.0), attr("beta2", nan), attr("beta1_power", 1.0), attr("beta2_power", 1.0),
        attr("beta1_power", -0.5), attr("eps", -1e-8), attr("eps", nan), attr("weight_decay", inf), attr("grad_scale", -1.0),
        attr("grad_scale", nan), attr("max_norm", nan),
        shape(0, (0,)), shape(0, (99,)), shape(2, (101,)), shape(3, (99,)), shape(4, (1,)),
    ]
    if clip:
        edits += [attr("max_norm", 0.0), attr("max_norm", -35.0), shape(1, (0,), F64)]
    if shadow:
        edits += [shape(5, (101,), B16)]                                                          # ns > n
    for i, e in enumerate(edits):
        assert rc(case, e) == ARG, i
    if clip:
        assert rc(case, shape(1, (1025,), F64)) == SIZE
    assert raw(case, both(*[shape(i, (2 ** 31,)) for i in (0, 2, 3, 4)])) == SIZE
    pairs = [(2, 0), (3, 0), (4, 0), (3, 2), (4, 2), (4, 3)] + ([(5, 0), (5, 2)] if shadow else []) + ([(2, 1)] if clip else [])
    for o, k in pairs:                                                                             # grad may alias no output, nor two outputs each other
        assert raw(case, same=[(o, k)]) == ARG, (o, k)


def test_grad_sumsq_semantic_refusals_return_the_documented_codes():
    ARG, SIZE = 2, 4
    for tag in ("[pool]", "[workspace]"):
        case = _case(tag, "md_grad_sumsq")
        for i, e in enumerate([shape(0, (0,)), shape(1, (2,), F64), shape(1, (0,), F64)]):
            assert rc(case, e) == ARG, i
        assert raw(case, shape(0, (2 ** 31,))) == SIZE
    assert rc(_case("[workspace]", "md_grad_sumsq"), shape(2, (7,), U8)) == SIZE


# ---------------------------------------------------------------------------------------------------- the reference, transcribed
def reference_adam(gradients, which, param, m, v, *, lr, beta1, beta2, beta1_power, beta2_power, eps, weight_decay, max_norm, grad_scale):
    """Adam.construct (custom_adam.py:602-668) for tensor `which` of `gradients` on torch float64: clip_grad_norm_ (:590-600, norm_type 2)
    over all of them, decay_weight (gradient + weight_decay param), scale_grad, then the dense branch of _run_opt_with_sparse
    (:188-222) without the scatter (every index once) -> (next_param, next_m, next_v), float64"""
    if max_norm is not None:
        total_norm = 0.0
        for grad in gradients:
            total_norm += torch.norm(grad) ** 2
        total_norm = total_norm ** (1.0 / 2)
        clip_coef = max_norm / (total_norm + 1e-6)
        if clip_coef < 1:
            gradients = [clip_coef * g for g in gradients]
    gradient = gradients[which]
    gradient = gradient + weight_decay * param
    gradient = gradient * grad_scale
    m = beta1 * m
    v = beta2 * v
    next_m = m + (1.0 - beta1) * gradient
    next_v = v + (1.0 - beta2) * torch.square(gradient)
    param_update = next_m / (torch.sqrt(next_v) + eps)
    lr_t = lr * (1 - beta2_power) ** 0.5 / (1 - beta1_power)
    next_param = param - lr_t * param_update
    return next_param, next_m, next_v


ADAM_CASES = [(clip, wd, gs) for clip in ("active", "inactive", None) for wd in (0.0, 1e-4) for gs in (1.0, 1.0 / 512)]


@pytest.mark.parametrize("clip,wd,gs", ADAM_CASES, ids=[f"clip {c}, wd {w}, scale {g:.4g}" for c, w, g in ADAM_CASES])
def test_contract_adam_equals_the_reference_transcription(clip, wd, gs):
    rng = np.random.default_rng(11)
    n = 500
    f32 = lambda a: np.asarray(a, np.float32)
    g, other = f32(rng.normal(0, 1, n)), f32(rng.normal(0, 1, 300))        # two tensors are clipped together (K = 2)
    scale = 100.0 / np.sqrt(tc.sumsq(g) + tc.sumsq(other))                  # global norm 100 ...
    g, other = f32(g * scale), f32(other * scale)
    max_norm = None if clip is None else (35.0 if clip == "active" else 1000.0)    # ... against 35 or 1000
    p, m, v = f32(rng.normal(0, 0.1, n)), f32(rng.normal(0, 0.01, n)), f32(rng.uniform(0, 1e-3, n))
    kw = dict(lr=np.float32(1e-3), beta1=np.float32(0.93), beta2=np.float32(0.999), beta1_power=np.float32(0.93) ** 3, beta2_power=np.float32(0.999) ** 3,
              eps=np.float32(1e-8), weight_decay=wd, grad_scale=gs)
    kw = {k: float(x) for k, x in kw.items()}
    ss = None if clip is None else [tc.sumsq(g), tc.sumsq(other)]
    if clip is not None:
        coef = max_norm / (np.sqrt(sum(ss)) + 1e-6)
        assert (coef < 1) == (clip == "active")
    got = tc.adam(g, p, m, v, sumsq=ss, max_norm=max_norm, rounded=False, **kw)
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    want = reference_adam([t64(g), t64(other)], 0, t64(p), t64(m), t64(v), max_norm=max_norm, **kw)
    worst = 0.0
    for a, b in zip(got, want):
        b = b.numpy()
        worst = max(worst, float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))))
    print(f"adam[clip {clip}, wd {wd}, scale {gs:.4g}]: worst relative difference {worst:.2e}")
    assert worst <= 1e-12
    r = tc.adam(g, p, m, v, sumsq=ss, max_norm=max_norm, **kw)
    assert all(x.dtype == np.float32 for x in r) and all(np.array_equal(x, y.astype(np.float32)) for x, y in zip(r, got))   # rounded once


def test_contract_adam_leaves_zero_state_under_a_zero_gradient():
    z = np.zeros(9, np.float32)
    z[1::2] = -0.0
    p = np.linspace(-1, 1, 9).astype(np.float32)
    kw = dict(lr=1e-3, beta1=0.9, beta2=0.999, beta1_power=0.9, beta2_power=0.999, eps=1e-8)
    for ss, mn in ((None, None), ([0.0], 35.0)):
        p2, m2, v2 = tc.adam(z, p, np.zeros(9, np.float32), np.zeros(9, np.float32), sumsq=ss, max_norm=mn, **kw)
        assert np.array_equal(p2, p) and not m2.any() and not v2.any() and not np.signbit(m2).any() and not np.signbit(v2).any()
    # with weight decay the parameter itself is the gradient: only a zero parameter stays
    p2, m2, v2 = tc.adam(z, np.zeros(9, np.float32), z * 0, z * 0, weight_decay=1e-4, **kw)
    assert not p2.any() and not np.signbit(p2).any() and not m2.any()
    want = reference_adam([torch.zeros(9, dtype=torch.float64)], 0, torch.from_numpy(p.astype(np.float64)), torch.zeros(9, dtype=torch.float64),
                          torch.zeros(9, dtype=torch.float64), weight_decay=0.0, max_norm=None, grad_scale=1.0, **kw)
    assert np.array_equal(want[0].numpy().astype(np.float32), p) and not want[1].any() and not want[2].any()


def test_contract_sumsq_is_the_float64_sum():
    g = np.array([3.0, -4.0, 1e-30, 1e30, 0.0, -0.0], np.float32)
    assert tc.sumsq(g[:2]) == 25.0 and tc.sumsq(g) == float(np.sum(g.astype(np.float64) ** 2)) and np.isfinite(tc.sumsq(g))


# ---------------------------------------------------------------------------------------------------- schedules
@pytest.mark.parametrize("name", ["a", "b"])
def test_one_cycle_equals_the_reference_bit_for_bit(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "one_cycle_vectors.npz"))
    args = z[name + "_args"]
    total, lr_max, div, pct, moms = int(args[0]), float(args[1]), args[2], float(args[3]), [float(args[4]), float(args[5])]
    div = int(div) if div == int(div) else float(div)
    assert (total, lr_max, div, pct, moms) == dict(a=(100, 1e-3, 10, 0.4, [0.95, 0.85]), b=(7, 3e-3, 25, 0.3, [0.9, 0.8]))[name]
    lrs, ms = optim.OneCycle(total, lr_max, div, pct, moms).get_lr()
    assert lrs.dtype == ms.dtype == np.float32 and lrs.shape == ms.shape == (total,)
    assert lrs.tobytes() == z[name + "_lrs"].tobytes() and ms.tobytes() == z[name + "_moms"].tobytes()
    cut = int(pct * total)
    assert lrs[0] == np.float32(lr_max / div) and lrs[cut] == np.float32(lr_max) and ms[0] == np.float32(moms[0]) and ms[cut] == np.float32(moms[1])
    assert (np.diff(lrs[:cut + 1]) > 0).all() and (np.diff(lrs[cut:]) < 0).all()


def test_exponential_decay_lr_is_the_documented_form():
    lr = optim.exponential_decay_lr(2e-4, 0.8, total_step=6 * 40, step_per_epoch=6, decay_epoch=15, is_stair=True)
    assert len(lr) == 240 and lr[0] == lr[6 * 15 - 1] == 2e-4 and lr[6 * 15] == 2e-4 * 0.8 and lr[-1] == 2e-4 * 0.8 ** 2
    smooth = optim.exponential_decay_lr(2e-4, 0.8, total_step=240, step_per_epoch=6, decay_epoch=15, is_stair=False)
    assert smooth[6] == 2e-4 * 0.8 ** (1 / 15) and smooth[5] == 2e-4 and all(a >= b for a, b in zip(smooth, smooth[1:]))
    assert "unpinned" in optim.exponential_decay_lr.__doc__.lower()
    with pytest.raises(ValueError):
        optim.exponential_decay_lr(2e-4, 0.8, 0, 6, 15)


@pytest.mark.parametrize("name", ["car", "ped_cycle", "tiny"])
def test_train_configs_carry_the_optimizer_and_the_schedule(name):
    from minddet.models import Config

    fn = "pointpillars_tiny_train.py" if name == "tiny" else f"pointpillars_{name}_xyres16_train.py"
    t = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", fn)).train_cfg
    assert t["optimizer"] == dict(type="Adam", weight_decay=0.0001)
    assert t["lr"] == dict(type="exponential_decay_lr", initial_learning_rate=0.0002, decay_rate=0.8, decay_epoch=15, is_stair=True,
                           max_num_epochs=80, batch_size=4)
    assert set(t["optimizer"]) - {"type"} <= set(optim.DEFAULT_OPTIMIZER)


# ---------------------------------------------------------------------------------------------------- the exclusion check
@pytest.mark.parametrize("name", list(train_cases.SIXTEEN_BIT_SHAPES))
def test_sixteen_bit_inputs_are_exact_in_fp32_and_exclude_a_bf16_dy(name):
    s = train_cases.SIXTEEN_BIT_SHAPES[name]
    x, dy = train_cases.data("sixteen-bit", s)
    kw = dict(cin=s["cin"], cout=s["cout"], x_c_off=s["x_c_off"], dy_c_off=s["dy_c_off"])
    want = tc.wgrad(x, dy, **kw)
    units = want["dw"] * 2.0 ** 20
    assert np.array_equal(units, np.round(units)) and np.abs(units).max() < 2 ** 24 and (want["absdw"] * 2.0 ** 20).max() < 2 ** 24
    assert np.array_equal(want["dw"].astype(np.float32).astype(np.float64), want["dw"])           # the exact result is an fp32 number
    assert np.array_equal(want["db"].astype(np.float32).astype(np.float64), want["db"])
    rounded = tc.wgrad(x, tc.bf16_round(dy), **kw)
    live = want["absdw"] > 0
    frac = float((rounded["dw"][live] != want["dw"][live]).mean())
    print(f"sixteen-bit[{name}]: {int(live.sum())} live elements, {100 * frac:.1f} % differ with dy rounded to bf16")
    assert live.sum() >= s["cin"] * s["cout"] * 0.9 and frac >= 0.9
    # the hi + lo split of dy into two bf16 terms would pass: 16 bits survive
    hi = tc.bf16_round(dy)
    lo = tc.bf16_round(dy - hi)
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), dy.astype(np.float64))
