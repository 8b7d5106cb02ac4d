"""CPU: the CenterNet training input without a GPU -- the ABI of include/minddet_hip_cnaug.h (the functions exported,
the semantic refusals answered before any device call, the ctypes mirrors laid out as the header says), the contract
tests/cnaug_contract.py against the reference's own values (tests/golden/cn_augment_vectors.npz, written by
tests/golden/gen_cn_augment.py from COCOHP.preprocess_fn and color_aug; tests/golden/cn_target_vectors.npz for the targets behind the
matrix), the sensitivity of the output to the order of the grey sum, det_ops.CenterNetAugment built from the train configs and its
refusals."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from minddet_amd import _lib, det_ops
from tests import cn_targets_contract as ct
from tests import cnaug_contract as cc
from tests import abi_header as ah
from tests.abi_cases import B16, I
from tests.abi_cases_cnaug import CASES, F64, CNImage, CNTransform
from tests.abi_derive import attr, both, edited, lib_handle, rc, refuse_single_defects, shape
from tests.test_cn_targets_cpu import fixture_case as targets_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = ah.header("minddet_hip_cnaug.h")
GOLD = os.path.join(ROOT, "tests", "golden", "cn_augment_vectors.npz")
SYMS = ["md_cn_aug_transform", "md_cn_aug_image"]
U8 = "uint8"
ARG, SIZE = 2, 4


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(GOLD)
    f = {k: z[k] for k in z.files}
    for v in f.values():
        v.setflags(write=False)
    return f


def attrs_of(f, i=None):
    """the keyword arguments of cc.transform / det_ops.cn_aug_transform for sample i of the fixture"""
    return dict(rand_crop=bool(f["rand_crop"][i]), scale=float(f["scale"]), shift=float(f["shift"]), flip_prop=float(f["flip_prop"]),
                input_hw=tuple(int(v) for v in f["input_hw"]), down_ratio=int(f["down_ratio"]))


def contract_transform(f, i):
    return cc.transform(f["size"][i:i + 1], f["draws"][i:i + 1], **attrs_of(f, i))


def test_header_declares_the_symbols_and_the_library_exports_them():
    assert ah.aot_symbols(HDR) == SYMS and '#include "minddet_hip.h"' in HDR
    for cite in ("dataset.py:278-315", "image.py:208-253", "image.py:229", "image.py:29-30", "DESIGN 9 item 5"):
        assert cite in HDR, cite
    assert "minddet_hip_cnaug.h" in open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    assert {c.sym for c in CASES} == set(SYMS) and len({c.id for c in CASES}) == len(CASES)
    lib = lib_handle()
    for s in SYMS:
        assert getattr(lib, s)(0, None, None, None, None, None, None) == 1      # wrong parameter count, before anything else
    assert not set(SYMS) & set(_lib.exported_symbols())                          # declared in the new header only


def test_ctypes_mirrors_and_limits_have_the_headers_layout():
    want = {"md_cn_aug_transform_attrs": ["int32_t rand_crop", "double scale, shift", "double flip_prop", "int32_t in_h, in_w", "int32_t down_ratio"],
            "md_cn_aug_image_attrs": ["int32_t out_h, out_w, pad_lo, pad_hi"]}
    for name, fields in want.items():
        assert ah.statements(name, HDR) == fields
    for got in (det_ops._CNAugTransformAttrs, CNTransform):       # int32, pad, three doubles, three int32, pad
        assert C.sizeof(got) == 48
        assert [(n, getattr(got, n).offset) for n, _ in got._fields_] == [("rand_crop", 0), ("scale", 8), ("shift", 16), ("flip_prop", 24),
                                                                          ("in_h", 32), ("in_w", 36), ("down_ratio", 40)]
    for got in (det_ops._CNAugImageAttrs, CNImage):
        assert C.sizeof(got) == 16 and [n for n, _ in got._fields_] == ["out_h", "out_w", "pad_lo", "pad_hi"]
    src = open(os.path.join(ROOT, "minddet_amd", "csrc", "cnaug.hip")).read()
    assert "sizeof(md_cn_aug_transform_attrs) == 48 && sizeof(md_cn_aug_image_attrs) == 16" in src
    defines = ah.defines(HDR)
    assert (defines["MD_CNAUG_MAX_BATCH"], defines["MD_CNAUG_GREY_CHUNK"]) == (det_ops.CNAUG_MAX_BATCH, 2048) == (65535, 2048)
    assert det_ops.cn_aug_image_workspace_bytes(2, 6, 10) == 32 and det_ops.cn_aug_image_workspace_bytes(16, 512, 512) == 8 * 16 * 129
    # (the chunk decides: 2048 pixels are one partial sum per sample, one more pixel is two)
    assert det_ops.cn_aug_image_workspace_bytes(1, 1, 2048) == 16 and det_ops.cn_aug_image_workspace_bytes(1, 1, 2049) == 24
    assert det_ops.CN_COLOUR_ORDERS == cc.ORDERS


def test_sampler_is_stated_once_and_shared():
    src = os.path.join(ROOT, "minddet_amd", "csrc")
    pre, cn, hdr = (open(os.path.join(src, n)).read() for n in ("preproc.hip", "cnaug.hip", "image_sample.h"))
    assert hdr.count("void sample_bilinear(") == 1 and "floorf" in hdr
    for text in (pre, cn):
        assert '#include "image_sample.h"' in text and "sample_bilinear(" in text and "floorf" not in text
    assert "block_sums<1>" in cn and "atomicAdd" not in cn and "hipMemset" not in cn


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_cnaug", case)


def test_semantic_refusals_return_the_documented_codes():
    nan, inf = float("nan"), float("inf")
    tr, tr_plain, img_ws, img_pool, img_plain = CASES
    for i, e in enumerate([shape(0, (2, 3), I), shape(0, (3, 2), I), shape(1, (3, 4), F64), shape(1, (2, 5), F64), shape(2, (2, 5)), shape(2, (3, 6)),
                           shape(3, (2, 5), F64), shape(3, (3, 6), F64), shape(4, (3,), I)]):
        assert rc(tr, e) == ARG, i
    for name, v in (("scale", nan), ("scale", inf), ("shift", nan), ("shift", -inf), ("flip_prop", nan), ("flip_prop", -0.01), ("flip_prop", 1.01),
                    ("down_ratio", 0), ("down_ratio", -4), ("in_h", 0), ("in_w", 0), ("in_h", 3)):          # (in_h below down_ratio: an empty map)
        assert rc(tr_plain, attr(name, v)) == ARG, (name, v)
    big = both(shape(0, (65536, 2), I), shape(1, (65536, 4), F64), shape(2, (65536, 6)), shape(3, (65536, 6), F64), shape(4, (65536,), I))
    assert rc(tr, big) == SIZE

    for i, e in enumerate([shape(0, (2, 8, 12, 4), U8), shape(0, (3, 8, 12, 3), U8), shape(1, (3, 2), I), shape(1, (2, 3), I), shape(2, (2, 5)), shape(2, (3, 6)),
                           shape(3, (5,)), shape(3, (7,)), shape(4, (2, 7), F64), shape(4, (3, 8), F64), shape(5, (2, 6, 10, 3), B16),
                           shape(5, (2, 6, 10, 16), B16), shape(5, (2, 7, 10, 8), B16), shape(5, (2, 6, 11, 8), B16), shape(5, (3, 6, 10, 8), B16),
                           attr("out_h", 0), attr("out_w", -1), attr("pad_lo", -1), attr("pad_hi", 1)]):
        assert rc(img_ws, e) == ARG, i
    assert rc(img_plain, shape(5, (2, 6, 10, 5), B16)) == ARG
    assert rc(img_ws, shape(6, (31,), U8)) == SIZE and rc(img_plain, shape(5, (2, 22, 26, 4), B16)) == ARG      # (the stem pads need the attrs)
    call = edited(img_pool, lambda c: None)               # (the shapes alone say B = 65536: the host blocks stay small, nothing is touched)
    for i, t in enumerate(call.case.operands):
        if i != 3:
            call.shapes[i] = [65536] + list(t.shape[1:])
    assert call.run(lib_handle()) == SIZE
    call = edited(img_plain, lambda c: None)              # a source of 2^30 elements
    call.shapes[0] = [2, 16384, 16384, 3]
    assert call.run(lib_handle()) == SIZE
    call = edited(img_plain, attr("out_h", 1 << 14))     # an output of 2^30 elements
    call.case.extra.out_w = 1 << 13
    call.shapes[5] = [2, 1 << 14, 1 << 13, 8]
    assert call.run(lib_handle()) == SIZE


def _raw_call(case, patch):
    """the case's call with one host block per operand; patch(params) edits the pointer array"""
    lib = lib_handle()
    ops = case.operands
    n = len(ops)
    bufs = [(C.c_char * 65536)() for _ in range(n)]
    params = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    for i, t in enumerate(ops):
        if t.null:
            params[i] = None
    patch(params)
    ndims = (C.c_int * n)(*[0 if t.null else len(t.shape) for t in ops])
    keep = [(C.c_int64 * max(len(t.shape), 1))(*t.shape) for t in ops]
    shapes = (C.POINTER(C.c_int64) * n)(*[C.cast(k, C.POINTER(C.c_int64)) for k in keep])
    dtypes = (C.c_char_p * n)(*[t.dtype.encode() for t in ops])
    return getattr(lib, case.sym)(n, params, ndims, shapes, dtypes, None, C.byref(case.extra))


def test_aliased_outputs_and_a_misaligned_workspace_are_refused():
    """an output at the address of an input or of another output, a workspace that is not 8-byte aligned: rc 2 before any device call"""
    for case, pairs in ((CASES[0], [(2, 0), (3, 1), (4, 0), (3, 2), (4, 3)]), (CASES[2], [(5, 0), (5, 1), (5, 2), (5, 3), (5, 4), (6, 5)])):
        for out, other in pairs:
            def alias(params, out=out, other=other):
                params[max(out, other)] = params[min(out, other)]
            assert _raw_call(case, alias) == ARG, (case.id, out, other)

    def shift(params):
        params[6] = params[6] + 4
    assert _raw_call(CASES[2], shift) == ARG


def test_fixture_carries_what_the_cases_promise():
    f = fixture()
    assert os.path.getsize(GOLD) < 300 * 1000 and len(f["size"]) == 7
    assert f["rand_crop"].tolist() == [True, False, True, False, True, False, True] and f["color_aug"].tolist() == [True] * 6 + [False]
    assert f["colour"][:6, 6].tolist() == [0, 1, 2, 3, 4, 5]                                  # all six orders
    assert bool(f["flipped"][0]) and f["rand_crop"][0] and f["size"][0].tolist() == [120, 200]   # narrower than 2 x 128: the border halves
    lo = det_ops.CenterNetAugment.get_border(128, torch.tensor([200, 120, 640, 64]))
    assert lo.tolist() == [64, 32, 128, 16] and 64 <= f["draws"][0, 1] < 200 - 64 and 32 <= f["draws"][0, 2] < 120 - 32
    d = f["draws"][1]
    assert not f["rand_crop"][1] and abs(d[0]) > 2 and abs(d[1]) < 2 and abs(d[2]) > 1      # the clips of c[0] and s active, of c[1] inactive
    assert not f["flipped"][1] and f["flipped"][3] and set(f["flipped"].tolist()) == {True, False}
    assert f["warped"].dtype == np.uint8 and f["warped"].shape == (7, 24, 40, 3) and f["inp"].shape == (7, 24, 40, 3) and f["inp"].dtype == np.float32
    assert f["c"].dtype == np.float32 and f["s"].dtype == np.float64 and f["draws"].shape == (7, 4) and f["trans_output"].shape == (7, 2, 3)
    assert (np.abs(f["colour"][:6, :3] - 1) <= 0.4).all() and not f["colour"][6].any()


@pytest.mark.parametrize("i", range(7))
def test_contract_c_s_and_flip_equal_the_reference_and_the_matrices_are_within_the_solve_bound(i):
    f = fixture()
    t = contract_transform(f, i)
    assert t["c"].dtype == np.float32 and np.array_equal(t["c"][0].view(np.int32), f["c"][i].view(np.int32))
    assert t["s"][0] == f["s"][i] and bool(t["flipped"][0]) == bool(f["flipped"][i])
    assert int(t["flip_width"][0]) == (int(f["size"][i, 1]) if f["flipped"][i] else 0)
    in_h, in_w = (int(v) for v in f["input_hw"])
    worst = 0.0
    for got, ref, dst_w in ((t["trans_out"][0], f["trans_output"][i], in_w // int(f["down_ratio"])), (t["trans_in"][0], f["trans_input"][i], in_w)):
        bound = cc.solve_bound(f["c"][i], f["s"][i], dst_w)
        err = np.abs(got - ref.ravel())
        assert (err <= bound).all(), (err, bound)
        worst = max(worst, float((err / bound).max()))
    print(f"sample {i}: worst matrix error / bound {worst:.3g}")
    # mat_in is the inverse of trans_in with the flip folded in: source -> input -> source is the identity (or the mirror)
    m, k = t["mat_in"][0].astype(np.float64), t["trans_in"][0]
    w = int(f["size"][i, 1])
    for px, py in ((0.0, 0.0), (float(in_w), float(in_h)), (7.0, 3.0)):
        sx, sy = m[0] * px + m[2], m[4] * py + m[5]
        if f["flipped"][i]:
            sx = w - 1 - sx
        assert abs(k[0] * sx + k[2] - px) < 1e-3 and abs(k[4] * sy + k[5] - py) < 1e-3


def _replayed_small_draws():
    """the draws tests/golden/gen_cn_targets.py's `small` case made: its seed, preprocess_fn's order (dataset.py:289-302)"""
    rs = np.random.RandomState(20260)
    d0 = [rs.randn(), rs.randn(), rs.randn(), rs.random_sample()]
    border = lambda size: int(det_ops.CenterNetAugment.get_border(128, torch.tensor([size]))[0])      # noqa: E731
    ch = rs.choice(np.arange(0.6, 1.4, 0.1))
    d1 = [ch, rs.randint(low=border(640), high=640 - border(640)), rs.randint(low=border(480), high=480 - border(480)), rs.random_sample()]
    return np.array([d0, d1], np.float64)


def test_targets_behind_the_contracts_matrix_reproduce_the_existing_fixture():
    """CenterNetTargets' arithmetic (tests/cn_targets_contract.py) fed the contract's trans_out against tests/golden/cn_target_vectors.npz,
    whose matrices are the reference's solve: the same outputs where the matrices agree bit for bit, post-affine boxes within the solve
    bound (plus the fp32 rounding of the stored box) elsewhere"""
    draws = _replayed_small_draws()
    runs = [("tiles", 0, (160, 288), np.zeros(4), dict(rand_crop=False, scale=0.0, shift=0.0, flip_prop=0.0), (160, 288)),
            ("small", 0, (120, 200), draws[0], dict(rand_crop=False, scale=0.4, shift=0.1, flip_prop=1.0), (96, 160)),
            ("small", 1, (480, 640), draws[1], dict(rand_crop=True, scale=0.4, shift=0.1, flip_prop=0.0), (96, 160))]
    equal = 0
    for name, b, hw, d, kw, in_hw in runs:
        inputs, tkw, ref = targets_case(name)
        t = cc.transform(np.array([hw]), d[None], input_hw=in_hw, down_ratio=4, **kw)
        assert int(t["flip_width"][0]) == int(inputs["flip_width"][b])
        got_m, ref_m = t["trans_out"][0].reshape(2, 3), inputs["trans_output"][b]
        bound = cc.solve_bound(t["c"][0], t["s"][0], in_hw[1] // 4).reshape(2, 3)
        assert (np.abs(got_m - ref_m) <= bound).all(), (name, b, got_m, ref_m)
        n = min(int(inputs["num_objects"][b]), tkw["max_objs"])
        post = ct.post_affine(inputs["bboxes"][b:b + 1, :n], got_m[None], t["flip_width"])
        want = inputs["post_boxes"][b:b + 1, :n]
        if np.array_equal(got_m, ref_m):
            equal += 1
            assert np.array_equal(post.view(np.int32), want.view(np.int32))
            if ref["hm"].shape[0] == 1:
                out = ct.assign(post, inputs["post_classes"][b:b + 1, :n], **tkw)
                for k in ct.KEYS:
                    assert np.array_equal(out[k], ref[k]), (name, k)
        else:
            xy = np.abs(ct.post_affine(inputs["bboxes"][b:b + 1, :n], None, t["flip_width"])).reshape(1, n, 2, 2)
            lim = (bound[:, 0] * xy[..., 0:1] + bound[:, 1] * xy[..., 1:2] + bound[:, 2]).reshape(1, n, 4) + 2 * cc.U * np.abs(want)
            assert (np.abs(post.astype(np.float64) - want) <= lim).all(), (name, b)
    print("matrices bit-equal to the recorded solve:", equal, "of", len(runs))
    assert equal >= 1


@pytest.mark.parametrize("i", range(6))
def test_colour_chain_is_within_the_forward_bound_of_the_reference(i):
    f = fixture()
    x32 = (f["warped"][i].astype(np.float32) / np.float32(255.0)).astype(np.float32)      # dataset.py:311
    got = cc.colour(x32, f["colour"][i], f["mean"], f["std"])
    bound = cc.colour_bound(x32, f["colour"][i], f["mean"], f["std"])
    err = np.abs(got["y"].astype(np.float64) - f["inp"][i].astype(np.float64))
    worst = float((err / bound).max())
    print(f"sample {i} (order {int(f['colour'][i, 6])}): worst colour error / bound {worst:.3f}, largest error {err.max():.3g}")
    assert (err <= bound).all(), worst
    assert worst > 0 and int(f["colour"][i, 6]) == i


def test_without_color_aug_the_normalisation_alone_is_bit_equal():
    f = fixture()
    x32 = (f["warped"][6].astype(np.float32) / np.float32(255.0)).astype(np.float32)
    y = ((x32 - f["mean"]) / f["std"]).astype(np.float32)
    assert np.array_equal(y.view(np.int32), f["inp"][6].view(np.int32))


def test_mean_sensitivity_of_the_bf16_output():
    """gs_mean summed in float64 in reversed order instead of exactly rounded: at most 1 in 10^4 bf16 outputs differ, each by 1 ulp"""
    f = fixture()
    total = diff = 0
    for i in range(6):
        x32 = (f["warped"][i].astype(np.float32) / np.float32(255.0)).astype(np.float32)
        g = cc.grey(x32)
        a = cc.bf16_bits(cc.colour(x32, f["colour"][i], f["mean"], f["std"])["y"])
        b = cc.bf16_bits(cc.colour(x32, f["colour"][i], f["mean"], f["std"], gs_mean=cc.reversed_sum(g) / g.size)["y"])
        n, worst = cc.bf16_differences(a, b)
        assert n * 10000 <= a.size and worst <= 1, (i, n, worst)
        total, diff = total + a.size, diff + n
    print(f"mean sensitivity: {diff} of {total} bf16 outputs differ")
    assert diff * 10000 <= total


def test_sampler_restatement_on_exact_cases():
    """where every product is exact the restatement is plain bilinear interpolation: the identity, a half-pixel shift, the mirror,
    the per-sample extent and the border rule"""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (6, 9, 3), dtype=np.uint8)
    ident = np.array([1, 0, 0, 0, 1, 0], np.float32)
    assert np.array_equal(cc.sample(img, (6, 9), ident, (6, 9)), img.astype(np.float32))
    half = cc.sample(img, (6, 9), np.array([1, 0, 0.5, 0, 1, 0], np.float32), (6, 9))
    want = (img[:, :-1].astype(np.float32) + img[:, 1:]) / 2
    assert np.array_equal(half[:, :-1], want) and np.array_equal(half[:, -1], img[:, -1].astype(np.float32) / 2)   # the last column: half border
    mirror = cc.sample(img, (6, 9), np.array([-1, 0, 8, 0, 1, 0], np.float32), (6, 9))
    assert np.array_equal(mirror, img[:, ::-1].astype(np.float32))
    small = cc.sample(img, (4, 5), ident, (6, 9))                                              # the sample's own extent: the rest is border
    assert np.array_equal(small[:4, :5], img[:4, :5].astype(np.float32)) and not small[4:].any() and not small[:, 5:].any()
    for bad in (np.nan, np.inf, -np.inf, 1e30):
        assert not cc.sample(img, (6, 9), np.array([1, 0, bad, 0, 1, 0], np.float32), (6, 9)).any()
    assert cc.bf16_bits(np.array([1.0, -0.0, 1.00390625, 1.01171875], np.float32)).tolist() == [0x3F80, 0x8000, 0x3F80, 0x3F82]   # ties to even


def test_train_configs_build_the_augmentation():
    from minddet.models import Config

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centernet", "centernet_r18_dcn_train.py"))
    a = cfg.train_cfg["augment"]
    assert (a["rand_crop"], a["scale"], a["shift"], a["flip_prop"], a["color_aug"]) == (True, 0.4, 0.1, 0.5, True)     # default_config.yaml:65-72
    f = fixture()
    assert np.array_equal(np.asarray(a["mean"], np.float32), f["mean"]) and np.array_equal(np.asarray(a["std"], np.float32), f["std"])
    assert np.array_equal(np.asarray(a["eig_val"], np.float32), f["eig_val"]) and np.array_equal(np.asarray(a["eig_vec"], np.float32), f["eig_vec"])
    aug = det_ops.CenterNetAugment.from_config(cfg)
    assert aug.input_hw == (512, 512) and aug.down_ratio == 4 and aug.rand_crop and aug.color_aug and aug.stem_layout
    assert (aug.scale, aug.shift, aug.flip_prop) == (0.4, 0.1, 0.5)
    assert np.array_equal(aug.eig_val.astype(np.float32), f["eig_val"]) and np.array_equal(np.asarray(aug.mean, np.float32), f["mean"])
    tiny = Config.fromfile(os.path.join(ROOT, "configs", "centernet", "centernet_tiny_train.py"))
    assert tiny.model == dict(type="CenterNet", depth=18, num_classes=5, head_conv=64, K=20, dcn=False)
    assert tiny.train_cfg["augment"] == a and tiny.train_cfg["loss"] == cfg.train_cfg["loss"]
    t = det_ops.CenterNetAugment.from_config(tiny)
    assert t.input_hw == (64, 96) and not t.stem_layout
    assert det_ops.CenterNetTargets.from_config(tiny).feature_map_size == (24, 16)


def test_augment_refused_options_and_the_draw_on_the_host():
    assert det_ops.CenterNetAugment((64, 96), 4, rot=0, aug_rot=0.0, rotate=0, keep_res=False).down_ratio == 4
    assert det_ops.CenterNetAugment((64, 96), (4, 4)).down_ratio == 4
    for kw in (dict(rot=15), dict(aug_rot=0.5), dict(rotate=1), dict(keep_res=True), dict(no_such_option=1), dict(down_ratio=(4, 8)),
               dict(flip_prop=1.5), dict(down_ratio=128)):
        with pytest.raises(ValueError):
            det_ops.CenterNetAugment((64, 96), **{"down_ratio": 4, **kw})
    doc = det_ops.CenterNetAugment.__doc__
    assert "NOT from numpy's" in doc and "keep_res" in doc
    # the distributions on the host generator (the device draw is tests/test_cn_augment_gpu.py's)
    sizes = torch.tensor([[120, 200], [480, 640], [1, 1], [64, 300]] * 50, dtype=torch.int32)
    g = torch.Generator().manual_seed(11)
    draws, colour = det_ops.CenterNetAugment((64, 96), 4).draw(sizes, g)
    steps = (draws[:, 0] - 0.6) / 0.1
    assert draws.dtype == colour.dtype == torch.float64 and set(steps.round().tolist()) == set(range(8))
    assert set(np.arange(0.6, 1.4, 0.1).tolist()) == set(draws[:, 0].tolist())               # np.arange's own values, bit for bit
    for col, k in ((1, 1), (2, 0)):
        lo = det_ops.CenterNetAugment.get_border(128, sizes[:, k].long())
        v = draws[:, col]
        assert bool(((v >= lo) & (v < torch.clamp(sizes[:, k] - lo, min=1)) & (v == v.round())).all())
    assert bool(((colour[:, :3] >= 0.6) & (colour[:, :3] <= 1.4)).all()) and set(colour[:, 6].tolist()) == {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}
    assert not colour[:, 7].any() and bool(((draws[:, 3] >= 0) & (draws[:, 3] < 1)).all())
    plain, none = det_ops.CenterNetAugment((64, 96), 4, rand_crop=False, color_aug=False).draw(sizes, g)
    assert none is None and 0.8 < float(plain[:, :3].std()) < 1.2
