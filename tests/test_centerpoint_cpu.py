"""CPU: the CenterPoint detector's model build (config, registry, head-tensor layout), the argument checks of md_conv2d_grouped (all before
any device call), the ISA audit of csrc/grouped.hip and the bbox_head weight import / export in both namings."""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from minddet_amd import _lib, graphs, nn_ops, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc.py")


def _detector(seed=7):
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(CFG)
    model = dict(cfg.model)
    return build_detector(dict(model, seed=seed), cfg.train_cfg, cfg.test_cfg), cfg


def test_config_builds_pointpillars_with_center_head():
    m, cfg = _detector()
    assert type(m) is graphs.PointPillars and type(m.bbox_head) is graphs.CenterHead and type(m.neck) is graphs.RPN
    assert m.neck.out_channels == 384 and m.bbox_head.in_channels == 384
    assert m.bbox_head.num_classes == [1, 2, 2, 1, 2, 2]
    assert cfg.test_cfg["nms"]["nms_post_max_size"] == 83 and cfg.test_cfg["out_size_factor"] == 4
    # the KITTI model keeps its own name free
    from minddet_amd.registry import DETECTORS
    assert DETECTORS.get("PointPillars") is graphs.PointPillars and DETECTORS.get("PointPillarsNet") is None


def test_reader_or_backbone_in_the_config_is_refused():
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(CFG)
    for extra in (dict(reader=dict(type="PillarFeatureNet")), dict(backbone=dict(type="PointPillarsScatter"))):
        with pytest.raises(ValueError, match="not part of this build"):
            build_detector(dict(cfg.model, **extra), cfg.train_cfg, cfg.test_cfg)


def test_head_tensor_layout():
    m, _ = _detector()
    h = m.bbox_head
    assert h.task_base == [0, 11, 23, 35, 46, 58] and h.head_channels == 70
    for t, base in enumerate(h.task_base):
        off = h.task_offsets(grouped=True)[t]
        assert list(off) == ["reg", "height", "dim", "rot", "vel", "hm"]
        assert [off[k] - base for k in off] == [0, 2, 3, 6, 8, 10]
    # A/B layout: branch i at channel 8 i
    ab = h.task_offsets(grouped=False)
    assert ab[0]["reg"] == 0 and ab[0]["hm"] == 40 and ab[5]["hm"] == 8 * 35
    assert len(h.branches()) == 36 and sum(c2.cout for _, _, _, c2 in h.branches()) == 70


def _grouped_rc(G=4, k=3, cin_g=64, couts=None, x_c_off=0, reserved0=0, nparam=4, N=1, H=8, W=8, C=None, Cy=16, R=None, w_k=None):
    """md_conv2d_grouped with fake non-null device pointers: every case below must be refused before the op touches them"""
    couts = couts or [2] * G
    C = C if C is not None else 64 * G
    R = R if R is not None else sum(couts)
    at = nn_ops._GroupedAttrs(k, 0, G, cin_g, x_c_off, reserved0)
    o = 0
    for g in range(min(G, 64)):
        at.cout[g], at.y_off[g], at.w_row[g] = couts[g], o, o
        o += couts[g]
    shapes = [[N, H, W, C], [R, w_k if w_k is not None else k * k * 64], [R], [N, H, W, Cy]][:nparam] + [[1]] * max(0, nparam - 4)
    dts = ["bfloat16", "bfloat16", "float32", "bfloat16"][:nparam] + ["bfloat16"] * max(0, nparam - 4)
    n = len(shapes)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    params = (ctypes.c_void_p * n)(*[0x100000 * (i + 1) for i in range(n)])
    ndims = (ctypes.c_int * n)(*[len(s) for s in shapes])
    bufs = [(ctypes.c_int64 * len(s))(*s) for s in shapes]
    shp = (ctypes.POINTER(ctypes.c_int64) * n)(*[ctypes.cast(b, ctypes.POINTER(ctypes.c_int64)) for b in bufs])
    dt = (ctypes.c_char_p * n)(*[d.encode() for d in dts])
    return lib.md_conv2d_grouped(n, params, ndims, shp, dt, None, ctypes.byref(at))


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="library not built")
def test_grouped_op_refuses_bad_arguments_without_a_device():
    ERR_NPARAM, ERR_ARG = 1, 2
    assert _grouped_rc(nparam=3) == ERR_NPARAM
    assert _grouped_rc(nparam=5) == ERR_NPARAM
    assert _grouped_rc(G=0, couts=[1]) == ERR_ARG                       # bad groups
    assert _grouped_rc(G=65, couts=[1] * 65, C=64 * 65) == ERR_ARG
    assert _grouped_rc(G=4, C=64 * 3) == ERR_ARG                       # groups past the input's channels
    assert _grouped_rc(cin_g=32) == ERR_ARG
    assert _grouped_rc(cin_g=128) == ERR_ARG
    assert _grouped_rc(couts=[2, 17, 1, 1], Cy=32) == ERR_ARG            # cout_g > 16
    assert _grouped_rc(couts=[2, 0, 1, 1]) == ERR_ARG
    assert _grouped_rc(x_c_off=4, C=64 * 4 + 8) == ERR_ARG             # misaligned x_c_off
    assert _grouped_rc(x_c_off=-8) == ERR_ARG
    assert _grouped_rc(reserved0=1) == ERR_ARG
    assert _grouped_rc(k=5) == ERR_ARG and _grouped_rc(k=2) == ERR_ARG
    assert _grouped_rc(w_k=64) == ERR_ARG                              # K of the packed weights != k * k * 64
    assert _grouped_rc(Cy=12) == ERR_ARG                               # Cy % 8
    assert _grouped_rc(couts=[8, 8, 8, 8], Cy=24) == ERR_ARG           # the last group's outputs past Cy
    assert _grouped_rc(R=5) == ERR_ARG                                 # rows past the packed weights


def test_grouped_attrs_layout_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "minddet_hip.h")).read()
    assert "#define MD_GROUPED_MAX_GROUPS 64" in hdr and "MD_CONV_KERNEL_GROUPED = 10" in hdr
    assert ctypes.sizeof(nn_ops._GroupedAttrs) == 4 * (6 + 3 * 64)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc + c++filt")
def test_grouped_kernel_passes_the_isa_audit():
    sys.path.insert(0, ROOT)
    from tools.isa_audit import audit

    rows, bad = audit(files=("grouped.hip",))
    assert not bad, "\n".join(bad)
    found = [(d, st) for d, st in rows if "md::grouped_conv_kernel" in d]
    assert len(found) == 2, [d for d, _ in rows]       # k = 3 and k = 1
    for d, st in found:
        assert st["mfma"] > 0 and st["spill"] == 0 and st["sgpr_spill"] == 0 and st["scratch"] == 0, (d, st)
        assert st["inner_exec_branches"] == 0, (d, st)   # no divergent branch between the first and the last MFMA
        assert st["vgpr"] <= 168, (d, st["vgpr"])       # three workgroups of four waves per CU (the LDS bound) stay resident


def test_pack_conv2d_grouped_folds_like_pack_conv():
    g = torch.Generator().manual_seed(0)
    convs = []
    for c in (1, 3, 2):
        w = torch.randn((c, 64, 3, 3), generator=g)
        b = torch.randn((c,), generator=g)
        bn = (torch.rand((c,), generator=g) + 0.5, torch.randn((c,), generator=g), torch.randn((c,), generator=g),
              torch.rand((c,), generator=g) + 0.5, 1e-5)
        convs.append((w, b, bn))
    pk = nn_ops.pack_conv2d_grouped(convs, y_offs=[5, 0, 9])
    assert tuple(pk.w.shape) == (6, 576) and tuple(pk.bias.shape) == (6,)
    assert pk.couts == [1, 3, 2] and pk.w_rows == [0, 1, 4] and pk.y_offs == [5, 0, 9]
    for (w, b, bn), r, c in zip(convs, pk.w_rows, pk.couts):
        pc = nn_ops.pack_conv(w, bias=b, bn=bn, pad=1, korder=0)
        assert torch.equal(pk.w[r:r + c], pc.w[:c, :576]) and torch.equal(pk.bias[r:r + c], pc.bias[:c])
    with pytest.raises(_lib.MindDetHipError):
        nn_ops.pack_conv2d_grouped([(torch.zeros((17, 64, 3, 3)), None, None)])
    with pytest.raises(_lib.MindDetHipError):
        nn_ops.pack_conv2d_grouped([(torch.zeros((2, 32, 3, 3)), None, None)])


def _same(a, b, naming):
    sa, sb = weights.center_head_state(a, naming=naming), weights.center_head_state(b, naming=naming)
    return sorted(sa) == sorted(sb) and all(np.array_equal(sa[k], sb[k]) for k in sa)


@pytest.mark.parametrize("naming", ["ms", "torch"])
def test_center_head_weights_round_trip(naming):
    a, b = _detector(1)[0].bbox_head, _detector(2)[0].bbox_head
    assert not _same(a, b, naming)
    st = weights.center_head_state(a, naming=naming)
    assert len(st) == 2 + 4 + 36 * (2 + 4 + 2)
    keys = set(st)
    bn = ("gamma", "beta", "moving_mean", "moving_variance") if naming == "ms" else ("weight", "bias", "running_mean", "running_var")
    assert {f"bbox_head.shared_conv.0.{n}" for n in ("weight", "bias")} <= keys
    assert {f"bbox_head.shared_conv.1.{n}" for n in bn} <= keys
    assert {f"bbox_head.tasks.5.hm.{i}.{n}" for i in (0, 3) for n in ("weight", "bias")} <= keys
    assert {f"bbox_head.tasks.5.hm.1.{n}" for n in bn} <= keys
    assert st["bbox_head.tasks.0.hm.3.weight"].shape == (1, 64, 3, 3) and st["bbox_head.tasks.1.hm.3.weight"].shape == (2, 64, 3, 3)
    assert np.all(st["bbox_head.tasks.0.hm.3.bias"] == np.float32(-2.19))
    if naming == "torch":
        st = dict(st, **{"bbox_head.shared_conv.1.num_batches_tracked": np.array(3)})
    assert weights.load_center_head(b, st, naming="auto") == []
    assert _same(a, b, naming)


def test_center_head_load_errors():
    h = _detector(1)[0].bbox_head
    st = weights.center_head_state(h)
    bad = dict(st)
    bad["bbox_head.tasks.2.dim.3.weight"] = np.zeros((2, 64, 3, 3), np.float32)
    with pytest.raises(ValueError):
        weights.load_center_head(_detector(2)[0].bbox_head, bad)
    del st["bbox_head.tasks.2.dim.3.bias"]
    with pytest.raises(KeyError):
        weights.load_center_head(_detector(2)[0].bbox_head, st)
    assert weights.load_center_head(_detector(2)[0].bbox_head, st, strict=False) == []
