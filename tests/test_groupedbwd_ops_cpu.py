"""CPU: the grouped conv-backward operators without a GPU -- the ABI of include/minddet_hip_groupedbwd.h (the two operators and the
workspace function exported, the semantic refusals answered before any device call), the judges of
tests/groupedbwd_contract.py against torch-CPU float64 autograd of F.conv2d(..., groups=G) with the per-group weights embedded in a
grouped conv of equal widths (k = 1 and 3, three images, couts 1 / 2 / 3), the mask rule, the channels no group covers, the frozen
BatchNorm that optim.CenterPointHeadTrainer.sync_modules writes back (nn_ops._fold_bn returns the master bit for bit) and the optimizer
blocks of the CenterPoint train configs."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from minddet_amd import _lib, det_ops, nn_ops, optim
from tests import groupedbwd_contract as gc, train_contract as tc
from tests import abi_header as ah
from tests.abi_cases import B16, U8, Grouped
from tests.abi_cases_groupedbwd import CASES, workspace_bytes
from tests.abi_derive import attr, both, item, lib_handle, raw, rc, refuse_single_defects, shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = ah.header("minddet_hip_groupedbwd.h")
OPS = ["md_conv2d_grouped_bwd_data", "md_conv2d_grouped_bwd_weight"]
ARG, SIZE = 2, 4


def _case(tag, sym):
    return next(c for c in CASES if c.sym == sym and c.tag == tag)


def test_header_declares_the_operators_and_the_library_exports_them():
    assert ah.aot_symbols(HDR) == OPS and '#include "minddet_hip_convbwd.h"' in HDR
    ws = re.findall(r"^extern int64_t (\w+_workspace_bytes)\((?:int64_t \w+(?:, )?)+\);", HDR, flags=re.M)
    assert ws == ["md_conv2d_grouped_bwd_weight_workspace_bytes"] and not re.search(r"^int64_t ", HDR, flags=re.M)
    assert re.search(r"^int md_conv2d_grouped_bwd_weight\(MD_AOT_ARGS\);\nextern int64_t md_conv2d_grouped_bwd_weight_workspace_bytes\(", HDR, flags=re.M)
    src = open(os.path.join(ROOT, "minddet_amd", "csrc", "convbwd.hip")).read()
    assert '#include "../../include/minddet_hip_groupedbwd.h"' in src
    assert "acquire_aligned(" in src and ".acquire(" not in src and not re.search(r"atomic\w*\(", src)
    assert {c.sym for c in CASES} == set(OPS) and len({c.id for c in CASES}) == len(CASES)
    lib = lib_handle()
    for sym in OPS:
        assert getattr(lib, sym)(0, None, None, None, None, None, None) == 1             # wrong parameter count, before anything else
    assert hasattr(lib, ws[0])
    # one valid row per optional-operand form
    assert {c.tag for c in CASES if c.sym == OPS[0]} == {f"[k{k}, {a}]" for k in (1, 3) for a in ("act", "no act")}
    assert {c.tag for c in CASES if c.sym == OPS[1]} == {f"[{w}, k{k}{d}]" for w in ("pool", "workspace") for k in (1, 3) for d in ("", ", no db")}
    for text in ("Ld(k, cout) = k k cout", "|dx - exact| <= Ld 2^-24 sum_{t, o} |dy w|", "bit for bit", "relu must be 0"):
        assert text in HDR, text
    defines = ah.defines(HDR)
    assert defines == dict(MD_GROUPED_BWD_TILE=64, MD_GROUPED_BWD_WALK=4)


def test_the_attribute_table_is_the_forward_calls():
    assert C.sizeof(nn_ops._GroupedAttrs) == C.sizeof(Grouped) == (6 + 3 * 64) * 4 and ah.layout(nn_ops._GroupedAttrs) == ah.layout(Grouped)
    main = ah.header("minddet_hip.h")
    body = "; ".join(ah.statements("md_conv2d_grouped_attrs", main))
    assert re.findall(r"int32_t (\w+)", body) == [n for n, _ in Grouped._fields_] and "#define MD_GROUPED_MAX_GROUPS 64" in main


def test_workspace_function_follows_the_headers_rule():
    """groups times the scratch of md_conv_bwd_weight for one group of cin 64 and one 16-row tile; -1 for a negative extent or a kernel
    the operator does not have; the Python function is the library's answer"""
    for P in (1, 15, 70, 300, 2145, 66048, 4 * 128 * 128):
        S = tc.slab_pixels(P)
        n = -(-P // S)
        for k in (1, 3):
            one = det_ops.conv_bwd_weight_workspace_bytes(P, 64, 16, k)
            assert one == 4 * n * 16 * (k * k * 64 + 1)
            for G in (1, 3, 36, 64):
                assert det_ops.conv2d_grouped_bwd_weight_workspace_bytes(P, G, k) == G * one, (P, G, k)
    assert workspace_bytes(3) == det_ops.conv2d_grouped_bwd_weight_workspace_bytes(15, 2, 3)
    f = lib_handle().md_conv2d_grouped_bwd_weight_workspace_bytes
    f.restype, f.argtypes = C.c_int64, [C.c_int64] * 3
    assert f(8, 8, 3) > 0 and f(-1, 8, 3) == -1 and f(8, -1, 3) == -1
    assert all(f(8, 8, k) == -1 for k in (-1, 0, 2, 5))
    with pytest.raises(_lib.MindDetHipError):
        det_ops.conv2d_grouped_bwd_weight_workspace_bytes(-1, 2, 3)
    src = open(os.path.join(ROOT, "minddet_amd", "det_ops.py")).read()
    body = re.search(r"^def conv2d_grouped_bwd_weight_workspace_bytes\(.*?\):\n((?:    .*\n)+)", src, flags=re.M).group(1)
    assert body.splitlines() == ['    return _lib.workspace_bytes("md_conv2d_grouped_bwd_weight", P, groups, k)']


# the refusals of the table, the same for both operators (rows: 6, dy channels: 8, the sliced tensor: 144 channels, x_c_off 8, 2 groups)
TABLE_EDITS = [
    attr("reserved0", 1), attr("reserved0", -1), attr("k", 0), attr("k", 2), attr("k", 5), attr("k", -3), attr("relu", 1), attr("relu", -1),
    attr("cin_g", 32), attr("cin_g", 0), attr("groups", 0), attr("groups", -1), attr("groups", 65), attr("groups", 3),
    attr("x_c_off", -8), attr("x_c_off", 17), attr("x_c_off", 24),
    item("cout", 0, 0), item("cout", 1, 17), item("cout", 1, -1), item("y_off", 0, -1), item("y_off", 0, 8), item("y_off", 1, 6),
    item("w_row", 0, -1), item("w_row", 1, 4), item("w_row", 0, 6),
]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_groupedbwd", case)


@pytest.mark.parametrize("tag", ["[k3, act]", "[k3, no act]", "[k1, act]"])
def test_dgrad_semantic_refusals_return_the_documented_codes(tag):
    case = _case(tag, OPS[0])
    k, act = case.extra.k, "no act" not in tag
    edits = TABLE_EDITS + [
        shape(0, (0, 3, 5, 8)), shape(0, (1, 3, 0, 8)), shape(3, (1, 3, 4, 144)), shape(3, (2, 3, 5, 144)), shape(3, (1, 3, 5, 135)),
        shape(1, (6, k * k * 64 + 64), B16), shape(1, (6, 64 if k == 3 else 576), B16), shape(1, (4, k * k * 64), B16),
    ]
    edits += [shape(2, (1, 3, 4, 144), B16), shape(2, (1, 3, 5, 135), B16)] if act else []
    for i, e in enumerate(edits):
        assert rc(case, e) == ARG, i
    for o in (0, 1) + ((2,) if act else ()):                                                       # dx at another operand's address
        assert raw(case, same=[(3, o)]) == ARG, o
    also = (lambda shp: shape(2, shp[:3] + (144,), B16)) if act else (lambda shp: (lambda c: None))
    huge = (2 ** 16, 2 ** 15, 1)                                                                   # P = 2^31
    assert raw(case, both(shape(0, huge + (8,)), shape(3, huge + (144,)), also(huge))) == SIZE
    big = (2 ** 14, 2 ** 10, 1)                                                                    # P = 2^24: dx of 2^31 elements and more
    assert raw(case, both(shape(0, big + (8,)), shape(3, big + (144,)), also(big))) == SIZE
    assert raw(case, shape(0, huge + (8,))) == ARG                                               # (dx no longer matches)


@pytest.mark.parametrize("tag", ["[pool, k3]", "[workspace, k3]", "[workspace, k1]", "[pool, k3, no db]"])
def test_wgrad_semantic_refusals_return_the_documented_codes(tag):
    case = _case(tag, OPS[1])
    k = case.extra.k
    edits = TABLE_EDITS + [
        item("w_row", 1, 0), both(item("w_row", 0, 3), item("cout", 0, 2)),                    # two groups that share a row of w
        shape(0, (0, 3, 5, 144), B16), shape(1, (1, 3, 0, 8)), shape(1, (1, 3, 4, 8)), shape(1, (2, 3, 5, 8)), shape(0, (1, 3, 5, 135), B16),
        shape(2, (6, k * k * 64 + 64)), shape(2, (6, 64 if k == 3 else 576)), shape(2, (4, k * k * 64)),
    ]
    edits += [shape(3, (5,)), shape(3, (8,))] if "no db" not in tag else []
    for i, e in enumerate(edits):
        assert rc(case, e) == ARG, i
    for o, kk in ((2, 0), (2, 1)) + (((3, 0), (3, 1), (3, 2)) if "no db" not in tag else ()):      # an output at another operand's address
        assert raw(case, same=[(o, kk)]) == ARG, (o, kk)
    huge = (2 ** 16, 2 ** 15, 1)
    assert raw(case, both(shape(0, huge + (144,), B16), shape(1, huge + (8,)))) == SIZE        # P = 2^31
    big = (2 ** 14, 2 ** 10, 1)
    assert raw(case, both(shape(0, big + (144,), B16), shape(1, big + (8,)))) == SIZE          # P = 2^24: x of 2^31 elements and more
    assert raw(case, shape(0, huge + (144,), B16)) == ARG                                        # (dy no longer matches)
    if "workspace" in tag:
        assert rc(case, shape(4, (workspace_bytes(k) - 1,), U8)) == SIZE                         # one byte short
        assert raw(case, shift=(4, 8)) == ARG                                                     # 8 bytes off a 16-byte boundary


# ---------------------------------------------------------------------------------------------------- the judges against autograd
def _autograd(pre, dy, w, tb, relu):
    """torch float64 autograd of F.conv2d(x, weight, groups=G) with every group widened to CM outputs (rows past cout zero):
    pre [N,H,W,C], dy [N,H,W,Cy], w [R, k k 64] -> (dw [R, k k 64], db [R], d sum(y dy) / d pre over the groups' channels)"""
    k, G, CM = tb["k"], len(tb["cout"]), max(tb["cout"])
    c0 = tb["x_c_off"]
    weight, dyf = np.zeros((G * CM, 64, k, k)), np.zeros(dy.shape[:3] + (G * CM,))
    for g in range(G):
        co, yo, wr = tb["cout"][g], tb["y_off"][g], tb["w_row"][g]
        weight[g * CM:g * CM + co] = w[wr:wr + co].reshape(co, k, k, 64).transpose(0, 3, 1, 2)
        dyf[..., g * CM:g * CM + co] = dy[..., yo:yo + co]
    pt = torch.from_numpy(np.ascontiguousarray(pre[..., c0:c0 + 64 * G])).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wt = torch.from_numpy(weight).requires_grad_(True)
    bt = torch.zeros(G * CM, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(torch.relu(pt) if relu else pt, wt, bt, stride=1, padding=k // 2, groups=G)
    (y * torch.from_numpy(dyf).permute(0, 3, 1, 2)).sum().backward()
    R = w.shape[0]
    dw, db = np.zeros((R, k * k * 64)), np.zeros(R)
    for g in range(G):
        co, wr = tb["cout"][g], tb["w_row"][g]
        dw[wr:wr + co] = wt.grad[g * CM:g * CM + co].permute(0, 2, 3, 1).reshape(co, -1).numpy()
        db[wr:wr + co] = bt.grad[g * CM:g * CM + co].numpy()
    return dw, db, pt.grad.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("k", [1, 3])
def test_the_judges_equal_float64_autograd_of_a_grouped_conv(k):
    rng = np.random.default_rng(k)
    N, H, W = 3, 5, 7
    tb = gc.table(k, (1, 2, 3), y_offs=(7, 0, 3), w_rows=(5, 0, 2), x_c_off=8)                     # unordered, gapped; row 6 owned by no group
    R, Cy, C = 7, 9, 8 + 192 + 5
    pre, dy, w = rng.normal(0, 1, (N, H, W, C)), rng.normal(0, 1, (N, H, W, Cy)), rng.normal(0, 1, (R, k * k * 64))
    x = np.maximum(pre, 0.0)
    dw, db, dx = _autograd(x, dy, w, tb, relu=False)
    got = gc.wgrad_grouped(x, dy, tb, R)
    assert np.abs(got["dw"] - dw).max() <= 1e-12 * np.abs(dw).max() and np.abs(got["db"] - db).max() <= 1e-12 * np.abs(db).max()
    assert got["live"].tolist() == [True] * 6 + [False] and not got["dw"][6].any() and not got["absdw"][6].any() and got["db"][6] == 0
    assert (got["absdw"] >= np.abs(got["dw"]) * (1 - 1e-12)).all()
    # every group alone is the judge of md_conv_bwd_weight for that group
    from tests import convbwd_contract as cc
    for g in range(3):
        one = cc.wgrad_kxk(x, dy, 64, tb["cout"][g], kernel=k, x_c_off=8 + 64 * g, dy_c_off=tb["y_off"][g])
        rows = slice(tb["w_row"][g], tb["w_row"][g] + tb["cout"][g])
        assert np.array_equal(one["dw"], got["dw"][rows]) and np.array_equal(one["db"], got["db"][rows])
    # the data gradient: without a mask, then through the ReLU (autograd of relu(pre): dx where pre > 0)
    plain = gc.dgrad_grouped(dy, w, tb, cdx=C)
    lo, hi = 8, 8 + 192
    assert np.abs(plain["dx"][..., lo:hi] - dx).max() <= 1e-12 * np.abs(dx).max() and plain["keep"][..., lo:hi].all()
    _, _, dpre = _autograd(pre, dy, w, tb, relu=True)
    masked = gc.dgrad_grouped(dy, w, tb, act=x.astype(np.float32), cdx=C)
    assert np.abs(masked["dx"][..., lo:hi] - dpre).max() <= 1e-12 * np.abs(dx).max() and 0.3 < masked["keep"][..., lo:hi].mean() < 0.7
    # the channels no group covers: nothing is said about them (0 in the judge, untouched on the device)
    for res in (plain, masked):
        assert res["covered"].tolist() == [False] * 8 + [True] * 192 + [False] * 5
        assert not res["dx"][..., ~res["covered"]].any() and not res["keep"][..., ~res["covered"]].any()
    assert sorted(set(plain["ld"][lo:hi].tolist())) == [k * k, 2 * k * k, 3 * k * k] and gc.dgrad_chain_length(3, 16) == 144
    assert np.array_equal(gc.dgrad_bound(plain), plain["ld"] * 2.0 ** -24 * plain["absdx"])


def test_the_mask_rule_at_its_edge_values():
    """+0, -0, a negative number, a NaN, the smallest positive bf16, 1, -inf, +inf in act: dx passes where act > 0 alone"""
    edge = np.array([0.0, -0.0, -1.0, np.nan, 9.2e-41, 1.0, -np.inf, np.inf], np.float32)
    act = np.tile(edge, 8).reshape(1, 1, 1, 64)
    tb = gc.table(1, (1,))
    res = gc.dgrad_grouped(np.ones((1, 1, 1, 1)), np.ones((1, 64)), tb, act=act)
    assert res["keep"].reshape(8, 8).tolist() == [[False, False, False, False, True, True, False, True]] * 8
    assert np.array_equal(res["dx"].reshape(-1), res["keep"].reshape(-1).astype(np.float64))


def test_a_tap_that_leaves_the_image_contributes_nothing():
    """a 1 x 1 image: only the centre tap meets it; two images: nothing crosses the seam"""
    tb = gc.table(3, (2,))
    w = np.arange(2 * 576, dtype=np.float64).reshape(2, 576) % 7 - 3
    dy = np.array([[1.0, 2.0], [-3.0, 5.0]]).reshape(2, 1, 1, 2)
    res = gc.dgrad_grouped(dy, w, tb)
    assert np.array_equal(res["dx"].reshape(2, 64), dy.reshape(2, 2) @ w[:, 4 * 64:5 * 64])


# ---------------------------------------------------------------------------------------------------- the trainer's host side
@pytest.mark.parametrize("eps", [1e-3, 1e-5])
def test_the_frozen_bn_written_back_folds_to_the_master_bit_for_bit(eps):
    g = torch.Generator().manual_seed(int(eps * 1e6))
    cout = 192
    mean, var = torch.randn(cout, generator=g) * 3, torch.rand(cout, generator=g) * 4
    var[:3] = torch.tensor([0.0, 1e-12, 1e6])
    master_w, master_b = torch.randn(cout, 64, 3, 3, generator=g), torch.randn(cout, generator=g)
    old = (torch.randn(cout, generator=g), torch.randn(cout, generator=g), mean, var, eps)
    bn = optim.identity_bn(old)
    assert bn[2] is mean and bn[3] is var and bn[4] == eps
    w, b = nn_ops._fold_bn(master_w, master_b, bn)
    assert int((w != master_w).sum()) == 0 and int((b != master_b).sum()) == 0
    assert w.dtype == torch.float32 and torch.equal(w, master_w) and torch.equal(b, master_b)
    # and the pack made from it is the bf16 rounding of the master
    pc = nn_ops.pack_conv(master_w, bias=master_b, bn=bn, pad=1, korder=0)
    cols = optim.pack_columns(pc)
    want = master_w.permute(0, 2, 3, 1).reshape(cout, 9, 64).to(torch.bfloat16)
    assert torch.equal(pc.w[:cout][:, cols.reshape(-1)].reshape(cout, 9, 64), want) and torch.equal(pc.bias[:cout], master_b)


@pytest.mark.parametrize("name", ["centerpoint_pp_nusc_train", "centerpoint_pp_tiny_points_train", "centerpoint_pp_tiny_head_train"])
def test_train_configs_carry_the_optimizer_and_the_schedule(name):
    from minddet.models import Config

    t = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", f"{name}.py")).train_cfg
    assert t["optimizer"] == dict(type="Adam", weight_decay=0.01, max_norm=35.0)
    assert t["lr_config"] == dict(type="OneCycle", lr_max=1e-3, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4)
    assert set(t["optimizer"]) - {"type"} <= set(optim.CENTERPOINT_OPTIMIZER)
    assert {k: optim.CENTERPOINT_OPTIMIZER[k] for k in ("type", "weight_decay", "max_norm")} == t["optimizer"]
    c = t["lr_config"]
    lrs, moms = optim.OneCycle(20, c["lr_max"], c["div_factor"], c["pct_start"], c["moms"]).get_lr()
    assert lrs[0] == np.float32(1e-4) and lrs[8] == np.float32(1e-3) and moms[0] == np.float32(0.95) and moms[8] == np.float32(0.85)


def test_the_trainer_refuses_what_is_not_built():
    class Stub:
        pass

    for cfg in (dict(type="SGD"), dict(type="Adam", momentum=0.9)):
        with pytest.raises(ValueError):
            optim.CenterPointHeadTrainer(Stub(), cfg)


def test_the_wrappers_refuse_before_the_library_is_asked():
    pk = nn_ops.pack_conv2d_grouped([(torch.zeros(2, 64, 3, 3), None, None)] * 2)
    dy, x = torch.zeros(1, 2, 2, 8), torch.zeros(1, 2, 2, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        det_ops.conv2d_grouped_bwd_data(dy.double(), pk)
    with pytest.raises(ValueError):
        det_ops.conv2d_grouped_bwd_data(dy, pk, act=x[:, :1])
    with pytest.raises(ValueError):
        det_ops.conv2d_grouped_bwd_data(dy, pk, act=x, x_c_off=8)
    with pytest.raises(ValueError):
        det_ops.conv2d_grouped_bwd_weight(x.float(), dy, pk)
    with pytest.raises(ValueError):
        det_ops.conv2d_grouped_bwd_weight(x, dy, pk, x_c_off=8)
    relu = nn_ops.pack_conv2d_grouped([(torch.zeros(2, 64, 3, 3), None, None)] * 2, relu=True)
    with pytest.raises(ValueError):
        det_ops.conv2d_grouped_bwd_weight(x, dy, relu)
