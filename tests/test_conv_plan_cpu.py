"""The conv dispatcher's launch plan (md_conv_plan), read on the CPU: which kernel instantiation, grid and workgroup each md_conv2d /
md_conv2d_head / md_conv1x1_dual call gets.  tests/golden/conv_plans.json holds every distinct call of one forward pass of Faster R-CNN
R50-FPN (b60 halves and the b120 batch on one stream, whose P2 layers run as image chunks), Mask R-CNN R101-FPN, YOLOv5s, YOLOv8l and
CenterNet (b32), with the launches a kernel trace recorded for it; the hand-written cases below cover the paths those models do not reach."""
import ctypes
import json
import os
import subprocess

import pytest

from minddet_amd import _lib, nn_ops
from tests.conv_contract import HALO, IGEMM, PINGPONG, STREAM, _struct, kernel_name, plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def conv(x, cout, k=3, stride=1, pad=None, relu=1, variant=0, korder=None, res=False, tune=None, res_up=False, lib_path=None, **adv):
    """md_conv2d on x [N,H,W,Cin] -> (rc, launches)"""
    pad = k // 2 if pad is None else pad
    n, h, w, cin = x
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    ct = nn_ops.cout_tile(cout)
    kpad = (k * k * cin + 63) // 64 * 64
    a = nn_ops._ConvAttrs(k, k, stride, pad, relu, variant)
    a.korder = (1 if k > 1 and cin % 64 == 0 else 0) if korder is None else korder
    a.res_upsample = int(res_up)
    if tune is not None:
        a.tune = tune
    y = [n, ho, wo, cout]
    for f, v in adv.items():
        setattr(a, f, v)
    if adv:
        a.adv, a.pad_top, a.pad_left, a.sub_h, a.sub_w, a.out_stride, a.cout = 1, pad, pad, ho, wo, 1, cout
        e = int("out_off_y" in adv or "out_off_x" in adv)   # room for a shifted output
        y = [n, ho + e, wo + e, adv.get("c_off", 0) + cout + 64]
    r = None if not res else ([n, (ho + 1) // 2, (wo + 1) // 2, cout] if res_up else [n, ho, wo, cout])
    return plan("md_conv2d", [list(x), [(cout + ct - 1) // ct * ct, kpad], [(cout + ct - 1) // ct * ct], r, y], a, lib_path=lib_path)


def one(x, cout, **kw):
    rc, ls = conv(x, cout, **kw)
    assert rc == 0 and len(ls) == 1, (rc, len(ls))
    return ls[0]


def test_plans_match_the_recorded_launches_of_five_models():
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "conv_plans.json")))["calls"]
    assert len(golden) > 300 and {e["workload"].split()[0] for e in golden} == {"faster_rcnn", "mask_rcnn", "yolov5s", "yolov8l", "centernet"}
    assert {e["op"] for e in golden} == {"md_conv2d", "md_conv2d_head", "md_conv1x1_dual"}
    assert any(len(e["launches"]) > 1 and e["op"] == "md_conv2d" for e in golden)   # image chunks (b120)
    cls = {"md_conv2d": nn_ops._ConvAttrs, "md_conv2d_head": nn_ops._ConvAttrs, "md_conv1x1_dual": nn_ops._DualAttrs}
    for e in golden:
        rc, ls = plan(e["op"], e["shapes"], _struct(cls[e["op"]], e["attrs"]), e["dtypes"])
        assert rc == 0, e
        got = [{"kernel": kernel_name(r), "grid": r.grid, "block": r.block, "lds": r.lds} for r in ls]
        assert got == e["launches"], (e["workload"], e["op"], e["shapes"])


def test_every_kept_variant_where_it_applies_and_where_it_falls_back():
    x3 = [8, 64, 64, 256]            # 3x3 256 -> 256 (korder 1)
    # 1 / 2 / 20: the 128x128 kernel register-staged / two / one LDS staging buffer
    r = one(x3, 256, variant=1, korder=0)
    assert conv(x3, 256, variant=1)[0] == 2         # korder-1 weights need the LDS-DMA kernels
    assert (r.family, r.mode, r.gen, r.single_buf, r.kernel_id) == (IGEMM, 0, 1, 0, 2)
    r = one(x3, 256, variant=2, korder=0)
    assert (r.family, r.mode, r.gen, r.single_buf) == (IGEMM, 2, 0, 0)
    r = one(x3, 256, variant=20, korder=0, relu=2)
    assert (r.family, r.mode, r.gen, r.single_buf) == (IGEMM, 2, 2, 1)
    r = one([1, 32, 32, 8], 128, variant=2)            # Cin % 64 != 0: the generic K walk
    assert (r.family, r.mode, r.gen, r.kernel_id) == (IGEMM, 1, 1, 4)
    # 11 / 27: the halo-reuse kernel with 128- / 64-cout tiles; else the double-buffered 128x128 (small-cout) kernel
    r = one(x3, 128, variant=11)
    assert (r.family, r.ct, r.one_halo, r.kernel_id) == (HALO, 128, 0, 5)
    r = one(x3, 64, variant=11)
    assert (r.family, r.ct, r.mode, r.single_buf) == (IGEMM, 64, 2, 0)
    r = one(x3, 64, variant=27)
    assert (r.family, r.ct, r.one_halo) == (HALO, 64, 1)
    r = one(x3, 64, k=1, variant=27)
    assert (r.family, r.ct, r.single_buf) == (IGEMM, 64, 0)
    # 15 / 22: the ping-pong kernel on either MFMA shape; else the double-buffered 128x128 kernel
    for v, mf in ((15, 0), (22, 1)):
        r = one(x3, 256, variant=v)
        assert (r.family, r.mf, r.pers, r.halo, r.gen, r.block, r.kernel_id) == (PINGPONG, mf, 0, 0, 0, 512, 1)
        r = one(x3, 128, variant=v)
        assert (r.family, r.mode, r.single_buf) == (IGEMM, 2, 0)
    # 30: conv1x1_stream_kernel; else auto
    r = one([8, 64, 64, 256], 1024, k=1, variant=30, res=True)
    assert (r.family, r.k, r.cb, r.nw, r.res, r.silu, r.kernel_id) == (STREAM, 256, 2, 4, 1, 0, 8)
    r = one([8, 64, 64, 512], 256, k=1, variant=30, relu=2)
    assert (r.family, r.k, r.cb, r.nw, r.res, r.silu) == (STREAM, 512, 1, 8, 0, 1)
    assert kernel_name(one(x3, 256, variant=30)) == kernel_name(one(x3, 256))
    # 32: the persistent ping-pong form; else auto (a residual)
    big = [16, 100, 168, 256]
    r = one(big, 256, variant=32)
    assert (r.family, r.pers, r.grid) == (PINGPONG, 1, 256)
    assert kernel_name(one(big, 256, variant=32, res=True)) == kernel_name(one(big, 256, res=True))
    # 33: auto without the persistent form (which auto picks on this long-K layer); where that form does not apply, auto
    assert one(big, 256).pers == 1 and one(big, 256, variant=33).pers == 0
    assert kernel_name(one(big, 256, variant=33, res=True)) == kernel_name(one(big, 256, res=True))
    # 34 / 35: auto with the HALO form wherever it applies / without it
    assert one(big, 256).halo == 0 and one(big, 256, variant=34).halo == 1
    p2 = [16, 200, 336, 256]          # 0.2 % idle tile pixels: auto takes the HALO form
    assert one(p2, 256).halo == 1 and one(p2, 256, variant=35).halo == 0
    assert kernel_name(one(x3, 256, k=1, variant=35)) == kernel_name(one(x3, 256, k=1))
    assert kernel_name(one(x3, 256, k=1, variant=34)) == kernel_name(one(x3, 256, k=1))
    # 36 / 37 / 38: the HALO form (32x32x16 / 16x16x32 / persistent); else the ping-pong kernel; else the generic kernel, one buffer
    for v, mf, pers in ((36, 0, 0), (37, 1, 0), (38, 1, 1)):
        r = one(big, 256, variant=v)
        assert (r.family, r.mf, r.halo, r.pers) == (PINGPONG, mf, 1, pers)
        r = one(big, 256, k=1, variant=v)
        assert (r.family, r.mf, r.halo, r.pers) == (PINGPONG, mf, 0, 0)
        r = one(big, 128, variant=v)
        assert (r.family, r.mode, r.single_buf) == (IGEMM, 2, 1)
    # 0: auto -- one staging buffer, two for a small grid with a long K loop (512->512 @20x20)
    r = one([1, 64, 64, 64], 128, k=1)
    assert (r.family, r.single_buf) == (IGEMM, 1)
    r = one([32, 20, 20, 512], 512, korder=0)
    assert (r.family, r.single_buf) == (IGEMM, 0)
    r = one([8, 64, 64, 64], 64)        # Cout <= 64: the 64-cout halo kernel
    assert (r.family, r.ct) == (HALO, 64)
    # sub-pixel / shifted outputs take the general epilogue; a channel range of a concat buffer keeps the plain one
    assert one([2, 32, 32, 64], 128, k=3, korder=0, c_off=64).gen == 0
    assert one([2, 32, 32, 64], 128, k=3, korder=0, out_off_y=1).gen == 1


def test_removed_unknown_and_diagnostic_codes_are_rejected():
    for v in (31, 39, 40, 7, 3, 41, -1, 17, 18, 19, 25, 26):
        rc, ls = conv([1, 32, 32, 256], 256, variant=v)
        assert rc == 2 and not ls, v


def _head(x, n_w2=32, variant=0, tune=None):
    a = nn_ops._ConvAttrs(3, 3, 1, 1, 1, variant)
    a.korder = 1
    if tune is not None:
        a.tune = tune
    n, h, w, cin = x
    return plan("md_conv2d_head", [list(x), [256, 9 * cin], [256], [n_w2, 256], [n_w2], [n, h, w, 16]], a)


def test_head_fused_and_two_launches():
    rc, ls = _head([2, 96, 96, 256])
    assert rc == 0 and len(ls) == 1
    assert (ls[0].family, ls[0].head, ls[0].gen, ls[0].grid, ls[0].sub) == (PINGPONG, 1, 0, 72, 0)   # one cout tile x 72 pixel tiles
    rc, ls = _head([2, 200, 336, 256])   # the HALO form from 90 % tile efficiency
    assert rc == 0 and len(ls) == 1 and ls[0].head == 1 and ls[0].halo == 1
    rc, ls = _head([1, 32, 32, 256])     # 4 pixel tiles: the conv into a temporary, then the 1x1 head on it
    assert rc == 0 and [r.sub for r in ls] == [0, 1]
    assert ls[0].head == 0 and (ls[1].family, ls[1].ct, ls[1].grid) == (IGEMM, 32, 8)
    rc, ls = _head([1, 32, 32, 256], n_w2=16)   # the fused kernel reads 16 rows; the two-launch form needs the padded 32
    assert rc == 2
    # image chunks of 4 and 3 images (2 MiB each): the first would fuse (64 pixel tiles), the last not (48) -> the whole call runs in the
    # two-launch form, both convs in the same chunks
    rc, ls = _head([7, 64, 64, 256], tune=nn_ops.ConvTune(chunk_limit=4 * 64 * 64 * 256 * 2 + 1))
    assert rc == 0 and [(r.sub, r.n0, r.nn, r.head) for r in ls] == [(0, 0, 4, 0), (0, 4, 3, 0), (1, 0, 4, 0), (1, 4, 3, 0)]


def test_image_chunks_with_a_lowered_chunk_limit():
    x = [5, 16, 16, 64]                  # 32 KiB per image, 3 images per chunk: chunks of 3 and 2 (even split)
    rc, ls = conv(x, 128, k=1, tune=nn_ops.ConvTune(chunk_limit=3 * 32768 + 100))
    assert rc == 0 and [(r.n0, r.nn) for r in ls] == [(0, 3), (3, 2)]
    assert ls[0].lds == ls[1].lds and ls[0].kernel_id == ls[1].kernel_id
    rc, ls = conv(x, 128, k=1)
    assert rc == 0 and [(r.n0, r.nn) for r in ls] == [(0, 5)]


def test_dual_on_both_sides_of_dual_pp_min_k():
    n, ho, wo = 4, 64, 64
    shapes = [[n, ho, wo, 256], [n, 2 * ho, 2 * wo, 512], [1024, 768], [1024], None, [n, ho, wo, 1024]]
    rc, ls = plan("md_conv1x1_dual", shapes, nn_ops._DualAttrs(2, 1, nn_ops.ConvTune()))
    assert rc == 0 and len(ls) == 1 and kernel_name(ls[0]) == "conv_pingpong_kernel<0, 0, 0, false, false, false>"
    rc, ls = plan("md_conv1x1_dual", shapes, nn_ops._DualAttrs(2, 1, nn_ops.ConvTune(dual_pp_min_k=1024)))
    assert rc == 0 and len(ls) == 1 and kernel_name(ls[0]) == "conv_igemm_kernel<256, 2, 2, 2, 2, 2, 0, 1>" and ls[0].single_buf == 1


def test_plan_argument_checks():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    n = ctypes.c_int(-1)
    assert lib.md_conv_plan(b"md_conv3d", 5, None, None, None, None, None, None, 0, ctypes.byref(n)) == 2
    assert lib.md_conv_plan(b"md_conv2d", 1, None, None, None, None, None, None, 0, ctypes.byref(n)) == 1
    rc, ls = conv([0, 16, 16, 64], 128)   # empty batch: no launch
    assert rc == 0 and not ls


def test_diagnostic_codes_in_the_diag_build():
    """The MD_DIAG library (tools/ only) keeps 17-19 / 25 / 26: the ping-pong timing ablations and stamp forms, 25 = 20 with stamps; where
    the ping-pong kernel does not apply, 17-19 / 26 fall back to the double-buffered 128x128 kernel."""
    csrc = os.path.join(ROOT, "minddet_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "-j8", "diag"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    diag = os.path.join(ROOT, "minddet_amd", "libminddet_hip_diag.so")
    x3 = [8, 64, 64, 256]
    for v, abl, mf in ((17, 1, 0), (18, 2, 0), (19, 4, 0), (26, 4, 1)):
        rc, ls = conv(x3, 256, variant=v, lib_path=diag)
        assert rc == 0 and kernel_name(ls[0]) == f"conv_pingpong_kernel<{abl}, {mf}, {0 if (abl, mf) == (4, 0) else 1}, false, false, false>", v
        rc, ls = conv(x3, 128, variant=v, lib_path=diag)
        assert rc == 0 and (ls[0].family, ls[0].mode, ls[0].single_buf) == (IGEMM, 2, 0), v
    rc, ls = conv(x3, 256, variant=25, korder=0, lib_path=diag)
    assert rc == 0 and (ls[0].family, ls[0].mode, ls[0].single_buf) == (IGEMM, 2, 1)
    assert conv(x3, 256, variant=31, lib_path=diag)[0] == 2
