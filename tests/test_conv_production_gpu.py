"""-m gpu: every production conv call of tests/golden/conv_plans.json (md_conv2d, md_conv2d_head, md_conv1x1_dual of Faster R-CNN b60 /
b120, Mask R-CNN, YOLOv5s, YOLOv8l and CenterNet) run through the C ABI exactly as recorded -- shapes, batch, the full attribute record
-- and compared over the WHOLE output tensor with the float64 reference of tests/conv_contract.py.

Each case first checks that the call takes its planned path: md_conv_plan reproduces the recorded launches, the call grows
md_conv2d_launch_count by that many launches and md_conv2d_last_kernel reports the last one's kernel.  The weights follow the header's
contract (a logical [cout, kh, kw, cin] weight packed in the attributes' K order, K and Cout zero padded), not the model packer.  The
output tensor starts as a NaN sentinel with a sentinel guard zone on both sides: every element the call must not write (channels
outside [c_off, c_off + cout), pixels out_stride / out_off do not address, the guard zones) keeps the sentinel bit for bit, and no
written element does.

Two data regimes per case:

exact     x and the residual are small bf16 integers (|x| <= 2, |res| <= 8), weights are drawn from {-1, 0, 1} 2^-s, the bias is an
          integer (|b| <= 3).  Every product and every partial sum of the fp32 accumulation is then a multiple of 2^-s below
          (2 K + 3 2^s) 2^-s in magnitude; the largest K of the records is 12544 (the box head's 7 x 7 x 256 FC) with s = 0, and
          s <= 4 where SiLU needs it, so |sum| 2^s < 2^15 < 2^24: exact in fp32 in any summation order.  (The head's second GEMM sums
          256 bf16 intermediates |t| < 2^13 (K = 2304) times {-1, 0, 1}: below 2^21.)  The expected output is the
          float64 result rounded to bf16 (round to nearest even) where the kernels round: conv + bias (+ SiLU) -> bf16, then + residual
          -> bf16, then ReLU; the head's 256-channel intermediate goes to bf16 after its ReLU.  ReLU and identity layers match bit for
          bit.  SiLU layers (s chosen so the pre-activation's spread is ~4) match bit for bit wherever the float64 SiLU lies more than
          delta |silu| from a bf16 rounding midpoint; elsewhere the kernel may round to either bf16 neighbour, and the output must
          equal the result of one of the two.  delta is derived in conv_contract.silu_delta from __expf and v_rcp_f32.
gaussian  x ~ N(0, 1) and weights ~ N(0, 1/K) rounded to bf16, bias ~ N(0, 1) fp32, residual ~ N(0, 1) bf16.  Every element must lie
          within conv_contract.gaussian_bound of the exact float64 result: half a bf16 ulp per rounding point plus c 2^-24 sum|x w| for
          the fp32 accumulation (c derived in conv_contract.accumulation_c).  The worst err / bound ratio of each case is printed
          (`pytest -s`).  Where K is small the half-ulp term dominates the bound and is attained at a bf16 tie, so ratios close to 1
          are expected there."""
import ctypes
import json
import os

import pytest
import torch

from minddet_amd import _lib, nn_ops
from tests import conv_contract as cc
from tests.conftest import has_gpu
from tests.conv_checks import GUARD, SENTINEL, Data, sentinel_out  # noqa: F401 (GUARD: test_sampling_gpu.py takes it from here)
from tests.conv_checks import check as _check
from tests.conv_checks import check_guards as _check_guards

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = json.load(open(os.path.join(ROOT, "tests", "golden", "conv_plans.json")))["calls"]
CHUNK_ELEMS = 1 << 27      # float64 elements per image chunk of the reference (1 GiB per tensor)


def _case_id(i, e):
    return f"{e['workload'].replace(' ', '_')}-{i}-{e['launches'][-1]['kernel'].replace(' ', '')}"


def _lib_fn(name, restype):
    f = getattr(_lib.lib(), name)
    f.restype = restype
    return f


def _sentinel_out(shape):
    return sentinel_out(shape, DEV)


def _Data(exact, seed):
    return Data(exact, seed, DEV)


def _call(op, tensors, e, n_launches, kernel_id):
    lc, lk = _lib_fn("md_conv2d_launch_count", ctypes.c_longlong), _lib_fn("md_conv2d_last_kernel", ctypes.c_int)
    for t, d in zip(tensors, e["dtypes"]):
        assert (t is None and d is None) or _lib._DT[str(t.dtype)].decode() == d
    l0 = lc()
    _lib.call(op, tensors, extra=cc._struct(cc.ATTR_CLS[op], e["attrs"]))
    assert lc() - l0 == n_launches and lk() == kernel_id, (lc() - l0, lk())
    torch.cuda.synchronize()


def _compare(got, pre, abs_sum, relu, res, c, exact):
    """one image chunk of one conv's output (float64 pre = conv + bias, abs_sum = sum|x w| + |b|) -> worst err / bound (0 if exact)"""
    gi = got.contiguous().view(torch.int16)
    if exact:
        if relu == 2:
            t, other, near = cc.silu_rounding(pre)
            want = cc.epilogue(pre, 2, res, t).to(torch.bfloat16).view(torch.int16)
            alt = cc.epilogue(pre, 2, res, other).to(torch.bfloat16).view(torch.int16)
            bad = (gi != want) & ~(near & (gi == alt))
        else:
            want = cc.epilogue(pre, relu, res).to(torch.bfloat16).view(torch.int16)
            bad = gi != want
        nbad = int(bad.sum())
        if nbad:
            idx = tuple(int(v) for v in bad.nonzero()[0])
            raise AssertionError(f"{nbad} of {bad.numel()} outputs differ; first at {idx}: got {got[idx].item()}, want "
                                 f"{want[idx].view(torch.bfloat16).item()}")
        return 0.0
    y, bnd = cc.gaussian_bound(pre, abs_sum, c, relu, res)
    err = (got.double() - y).abs()
    assert bool(torch.isfinite(err).all()), "non-finite output"
    ratio = err / bnd
    worst = float(ratio.max())
    if worst > 1:
        idx = tuple(int(v) for v in (ratio > 1).nonzero()[0])
        raise AssertionError(f"{int((ratio > 1).sum())} outputs past the bound; first at {idx}: got {got[idx].item()}, want "
                             f"{y[idx].item()} +- {bnd[idx].item()}")
    return worst


def _chunks(n, per_image):
    nb = max(1, CHUNK_ELEMS // max(per_image, 1))
    return [(i, min(n, i + nb)) for i in range(0, n, nb)]


def _run_conv2d(e, d):
    x_s, w_s, b_s, r_s, y_s = e["shapes"]
    a = e["attrs"]
    g = cc.conv_geometry(e["shapes"], a)
    x = d.act(x_s)
    wl = d.weight((g.cout, g.kh, g.kw, g.cin), g.k, silu=a["relu"] == 2)
    w = cc.pack_weight(wl, a["korder"], w_s[1], w_s[0])
    b = d.bias(g.cout, b_s[0])
    r = None if r_s is None else d.act(r_s, hi=8)
    y, flat = _sentinel_out(y_s)
    _call("md_conv2d", [x, w, b, r, y], e, len(e["launches"]), e["kernel_id"])
    _check_guards(flat)
    mask = cc.written_mask(g, DEV)
    yi = y.view(torch.int16)
    c = cc.accumulation_c(g.k + 1)
    worst = 0.0
    n = x_s[0]
    for n0, n1 in _chunks(n, max(x_s[1] * x_s[2] * g.cin, g.sub_h * g.sub_w * g.cout, y_s[1] * y_s[2] * y_s[3])):
        yc = yi[n0:n1]
        assert bool((yc[:, ~mask] == SENTINEL).all()), "write outside the call's output region"
        got = cc.out_view(y[n0:n1], g)
        assert not bool((got.view(torch.int16) == SENTINEL).any()), "output element left unwritten"
        pre = cc.conv_sum(x[n0:n1], wl, g) + b[:g.cout].double()
        absum = None if d.exact else cc.conv_sum(x[n0:n1], wl, g, absolute=True) + b[:g.cout].double().abs()
        res = cc.residual_values(None if r is None else r[n0:n1], a, g)
        worst = max(worst, _compare(got, pre, absum, a["relu"], res, c, d.exact))
    return worst


def _run_head(e, d):
    x_s, w_s, b_s, w2_s, b2_s, y_s = e["shapes"][:6]
    a = e["attrs"]
    g = cc.conv_geometry(e["shapes"][:6], a)
    x = d.act(x_s)
    wl = d.weight((256, g.kh, g.kw, g.cin), g.k)
    w = cc.pack_weight(wl, a["korder"], w_s[1], w_s[0])
    b = d.bias(256, b_s[0])
    w2l = d.weight((16, 256), 256)
    w2 = torch.full(w2_s, float("nan"), dtype=torch.bfloat16, device=DEV)   # rows >= 16 are ignored: garbage
    w2[16:].view(torch.int16)[::2] = 0x4F80                                     # (NaN and 2^32 alternating)
    w2[:16] = w2l
    b2 = d.bias(16, b2_s[0])
    y2, flat = _sentinel_out(y_s)
    tensors = [x, w, b, w2, b2, y2] + [None] * (len(e["shapes"]) - 6)
    _call("md_conv2d_head", tensors, e, len(e["launches"]), e["kernel_id"])
    _check_guards(flat)
    worst = 0.0
    for n0, n1 in _chunks(x_s[0], max(x_s[1] * x_s[2] * g.cin, g.sub_h * g.sub_w * 256)):
        ref = cc.reference_head(x[n0:n1], wl, b, w2l, b2, g, exact=d.exact)
        worst = max(worst, _check(y2[n0:n1], ref, d.exact))
    return worst


def _run_dual(e, d):
    xa_s, xb_s, w_s, b_s, r_s, y_s = e["shapes"]
    a = e["attrs"]
    assert r_s is None
    k = xa_s[3] + xb_s[3]
    cout = y_s[3]
    xa, xb = d.act(xa_s), d.act(xb_s)
    wl = d.weight((cout, k), k)
    w = cc.pack_weight(wl[:, None, None, :], 0, w_s[1], w_s[0])
    b = d.bias(cout, b_s[0])
    y, flat = _sentinel_out(y_s)
    _call("md_conv1x1_dual", [xa, xb, w, b, None, y], e, len(e["launches"]), e["kernel_id"])
    _check_guards(flat)
    worst = 0.0
    for n0, n1 in _chunks(xa_s[0], max(xb_s[1] * xb_s[2] * xb_s[3], y_s[1] * y_s[2] * y_s[3])):
        ref = cc.reference_dual(xa[n0:n1], xb[n0:n1], wl, b[:cout], a["stride_b"], a["relu"], exact=d.exact)
        worst = max(worst, _check(y[n0:n1], ref, d.exact))
    return worst


RUN = {"md_conv2d": _run_conv2d, "md_conv2d_head": _run_head, "md_conv1x1_dual": _run_dual}


@pytest.mark.parametrize("i", range(len(CALLS)), ids=[_case_id(i, e) for i, e in enumerate(CALLS)])
def test_production_call(i):
    e = dict(CALLS[i])
    rc, ls = cc.plan(e["op"], e["shapes"], cc._struct(cc.ATTR_CLS[e["op"]], e["attrs"]), e["dtypes"])
    assert rc == 0 and [{"kernel": cc.kernel_name(r), "grid": r.grid, "block": r.block, "lds": r.lds} for r in ls] == e["launches"]
    e["kernel_id"] = ls[-1].kernel_id
    worst = 0.0
    for exact in (True, False):
        worst = max(worst, RUN[e["op"]](e, _Data(exact, 1000 + 2 * i + int(exact))))
        torch.cuda.empty_cache()
    print(f"worst gaussian err/bound {_case_id(i, e)}: {worst:.4f}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the fused conv kernels at production shapes: md_stem_pool, md_stem_conv and md_bottleneck as the models built from configs/ call them
# ---------------------------------------------------------------------------------------------------------------------------------
FUSED = ("md_stem_pool", "md_stem_conv", "md_bottleneck")
# (workload, config, batch, what runs): the batches are conv_plans.json's workloads; the image size is the config's data.input_hw
MODELS = [("faster_rcnn b60", "configs/faster_rcnn/faster_rcnn_r50_fpn.py", 60, "backbone"),
          ("faster_rcnn b120", "configs/faster_rcnn/faster_rcnn_r50_fpn.py", 120, "backbone"),
          ("mask_rcnn b32", "configs/mask_rcnn/mask_rcnn_r101_fpn.py", 32, "backbone"),
          ("yolov5s b32", "configs/yolov5/yolov5s.py", 32, "forward"),
          ("yolov8l b32", "configs/yolov8/yolov8l.py", 32, "forward")]


def _fields(s):
    if s is None:
        return None
    return {f: (_fields(getattr(s, f)) if isinstance(getattr(s, f), ctypes.Structure) else getattr(s, f)) for f, _ in s._fields_}


def _fused_calls(config, batch, what):
    """the distinct md_stem_pool / md_stem_conv / md_bottleneck calls (op, shapes, attrs) of one pass of the model built from config"""
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(os.path.join(ROOT, config))
    m = build_detector(cfg.model, cfg.train_cfg, cfg.test_cfg).to(DEV)
    h, w = cfg.data["input_hw"]
    x4 = torch.zeros((batch, h + 16, w + 16, 4), dtype=torch.bfloat16, device=DEV)
    x4[:, cc.STEM_LO:cc.STEM_LO + h, cc.STEM_LO:cc.STEM_LO + w, :3] = torch.randn((batch, h, w, 3), device=DEV).to(torch.bfloat16)
    calls, orig = [], _lib.call

    def record(name, tensors, extra=None, stream=None):
        if name in FUSED:
            c = (name, [None if t is None else list(t.shape) for t in tensors], _fields(extra))
            if c not in calls:
                calls.append(c)
        return orig(name, tensors, extra=extra, stream=stream)

    _lib.call = record
    try:
        m.backbone(x4) if what == "backbone" else m.forward(x4)
        torch.cuda.synchronize()
    finally:
        _lib.call = orig
    del m, x4
    torch.cuda.empty_cache()
    return calls


def _stem_input(d, shape):
    """a stem-layout batch: the image at (7, 7), zero border and channel 3 (the header's input contract)"""
    x4 = torch.zeros(shape, dtype=torch.bfloat16, device=DEV)
    cc.stem_image(x4)[...] = d.act(list(cc.stem_image(x4).shape))
    return x4


def _run_fused(op, shapes, attrs, d):
    lc, lk = _lib_fn("md_conv2d_launch_count", ctypes.c_longlong), _lib_fn("md_conv2d_last_kernel", ctypes.c_int)
    y_s = shapes[-1]
    y, flat = _sentinel_out(y_s)
    if op == "md_bottleneck":
        x_s, w1_s, _, w2_s, w3_s, _, r_s, wd_s, _, _ = shapes
        cin = x_s[3]
        x = d.act(x_s, hi=1)
        w1l, w2l, w3l = d.weight((64, cin), cin), d.weight((64, 3, 3, 64), 576), d.weight((256, 64), 64)
        b1, b2, b3 = d.bias(64, 64), d.bias(64, 64), d.bias(256, 256)
        r = None if r_s is None else d.act(r_s, hi=1)
        wdl, bd = (d.weight((256, 64), 64), d.bias(256, 256)) if wd_s is not None else (None, None)
        tensors = [x, w1l, torch.cat([b1, b2]), cc.pack_weight(w2l, 0, 576, 64), w3l, b3, r, wdl, bd, y]
        extra = None if attrs is None else cc._struct(nn_ops.ConvTune, attrs)
        l0 = lc()
        _lib.call(op, tensors, extra=extra)
        limit = (attrs or {}).get("chunk_limit") or (1 << 31) - (1 << 16)
        assert lk() == 7 and (lc() - l0 > 1) == (x.numel() * 2 > limit), (lk(), lc() - l0)   # MD_CONV_KERNEL_BOTTLENECK, image chunks
        ref = lambda n0, n1: cc.reference_bottleneck(x[n0:n1], w1l, b1, w2l, b2, w3l, b3, None if r is None else r[n0:n1], wdl, bd,
                                                     exact=d.exact)
        per = x_s[1] * x_s[2] * 256 * 4
    else:
        x4_s, w_s, b_s, _ = shapes
        x4 = _stem_input(d, x4_s)
        if op == "md_stem_pool":
            wl = d.weight((64, 7, 7, 3), 147)
            w, b = cc.pack_stem_pool(wl), d.bias(64, 64)
            ref = lambda n0, n1: cc.reference_stem_pool(x4[n0:n1], wl, b, exact=d.exact)
        else:
            k, act = attrs["kh"], attrs["act"]
            wl = d.weight((w_s[0], k, k, 3), k * k * 3, silu=act == 2)
            w, b = cc.pack_stem_conv(wl), d.bias(w_s[0], w_s[0])
            ref = lambda n0, n1: cc.reference_stem_conv(x4[n0:n1], wl, b, act, exact=d.exact)
        _lib.call(op, [x4, w, b, y], extra=None if attrs is None else cc._struct(nn_ops._StemConvAttrs, attrs))
        per = (x4_s[1] * x4_s[2]) // 4 * 64 * 4
    torch.cuda.synchronize()
    _check_guards(flat)
    worst = 0.0
    for n0, n1 in _chunks(y_s[0], per):
        got, want = y[n0:n1], ref(n0, n1)
        if op == "md_stem_conv" and d.exact:     # the float64 pre-activation: SiLU's rounding judged as for md_conv2d
            worst = max(worst, _compare(got, want, None, attrs["act"], None, 0.0, True))
        else:
            worst = max(worst, _check(got, want, d.exact))
    return worst


@pytest.mark.parametrize("workload,config,batch,what", MODELS, ids=[m[0].replace(" ", "_") for m in MODELS])
def test_fused_production_calls(workload, config, batch, what):
    calls = _fused_calls(config, batch, what)
    ops = {c[0] for c in calls}
    assert ops == ({"md_stem_pool", "md_bottleneck"} if what == "backbone" else {"md_stem_conv"}), ops
    for j, (op, shapes, attrs) in enumerate(calls):
        worst = 0.0
        for exact in (True, False):
            worst = max(worst, _run_fused(op, shapes, attrs, _Data(exact, 7000 + 2 * j + int(exact))))
            torch.cuda.empty_cache()
        print(f"worst gaussian err/bound {workload} {op} {shapes[0]}: {worst:.4f}")
