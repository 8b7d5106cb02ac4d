"""CPU: the conv-backward operators without a GPU -- the ABI of include/minddet_hip_convbwd.h (the two operators and the workspace function
exported, the semantic refusals answered before any device call, the ctypes mirrors laid out as the header
says), the judges of tests/convbwd_contract.py against torch-CPU float64 autograd of F.conv2d (weight, bias and input gradients for
k = 1 and 3 over several images: the contract is pinned independently of a hand derivation), the column-order map against
nn_ops.pack_conv, optim.multi_epochs_decay_lr by hand-computed values and the two CenterNet train configs' optimizer blocks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from minddet_amd import _lib, det_ops, nn_ops, optim
from tests import convbwd_contract as cc, train_contract as tc
from tests import abi_header as ah
from tests.abi_cases import B16, U8
from tests.abi_cases_convbwd import CASES, Block, Conv1x1BwdData, ConvBwd, workspace_bytes
from tests.abi_derive import attr, both, edited, lib_handle, raw, rc, refuse_single_defects, shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = ah.header("minddet_hip_convbwd.h")
OPS = ["md_conv_bwd_weight", "md_conv1x1_bwd_data"]
ARG, SIZE = 2, 4


def _case(tag, sym):
    return next(c for c in CASES if c.sym == sym and c.tag == tag)


def test_header_declares_the_operators_and_the_library_exports_them():
    assert ah.aot_symbols(HDR) == OPS and '#include "minddet_hip_train.h"' in HDR
    ws = re.findall(r"^extern int64_t (\w+_workspace_bytes)\((?:int64_t \w+(?:, )?)+\);", HDR, flags=re.M)
    assert ws == ["md_conv_bwd_weight_workspace_bytes"] and not re.search(r"^int64_t ", HDR, flags=re.M)
    assert re.search(r"^int md_conv_bwd_weight\(MD_AOT_ARGS\);\nextern int64_t md_conv_bwd_weight_workspace_bytes\(", HDR, flags=re.M)
    assert "minddet_hip_convbwd.h" in open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "minddet_amd", "csrc", "convbwd.hip")).read()
    assert "acquire_aligned(" in src and ".acquire(" not in src and not re.search(r"atomic\w*\(", src)
    assert {c.sym for c in CASES} == set(OPS) and len({c.id for c in CASES}) == len(CASES)
    lib = lib_handle()
    for sym in OPS:
        assert getattr(lib, sym)(0, None, None, None, None, None, None) == 1             # wrong parameter count, before anything else
    assert hasattr(lib, ws[0])
    # one valid row per optional-operand form
    assert {c.tag for c in CASES if c.sym == OPS[0]} == {f"[{w}, k{k}{d}]" for w in ("pool", "workspace") for k in (1, 3) for d in ("", ", no db")} | \
        {"[pool, k3, one block]"}
    assert {c.tag for c in CASES if c.sym == OPS[1]} == {"[act]", "[no act]"}
    for text in ("L(P) = S / 4 + 3 + ceil(n / 8) + 7", "Ld(cout) = cout", "bit for bit"):
        assert text in HDR, text


def test_workspace_function_follows_the_headers_formula():
    defines = ah.defines(HDR)
    assert (defines["MD_CONV_BWD_MAX_CIN_K1"], defines["MD_CONV_BWD_MAX_CIN_K3"], defines["MD_CONV_BWD_MAX_COUT"], defines["MD_CONV_BWD_MAX_BLOCKS"]) == \
        (1024, 256, 256, 4)
    assert (defines["MD_CONV1X1_BWD_DATA_MAX_CIN"], defines["MD_CONV1X1_BWD_DATA_MAX_COUT"]) == (1024, 256)
    for P, cin, cout in ((1, 8, 1), (15, 8, 3), (70, 8, 20), (300, 64, 192), (2145, 384, 20), (66048, 8, 1), (16 * 128 * 128, 64, 192)):
        S = tc.slab_pixels(P)
        n, R = -(-P // S), -(-cout // 16) * 16
        for k in (1, 3):
            if k == 3 and cin > 256:
                continue
            assert det_ops.conv_bwd_weight_workspace_bytes(P, cin, cout, k) == 4 * n * R * (k * k * cin + 1), (P, cin, cout, k)
        assert det_ops.conv_bwd_weight_workspace_bytes(P, cin, cout, 1) == det_ops.conv1x1_bwd_weight_workspace_bytes(P, cin, cout)
    assert workspace_bytes(3) == det_ops.conv_bwd_weight_workspace_bytes(15, 8, 3, 3)
    f = lib_handle().md_conv_bwd_weight_workspace_bytes
    f.restype, f.argtypes = C.c_int64, [C.c_int64] * 4
    assert f(8, 8, 8, 3) > 0 and all(f(*[-1 if j == k else 8 for j in range(3)], 3) == -1 for k in range(3))     # a negative extent answers -1
    assert f(8, 8, 8, 2) == -1 and f(8, 8, 8, -1) == -1                                                        # so does a kernel the op does not have
    with pytest.raises(_lib.MindDetHipError):
        det_ops.conv_bwd_weight_workspace_bytes(-1, 8, 1, 3)


def test_ctypes_mirrors_have_the_headers_layout():
    block = ah.struct_of("md_conv_bwd_block", HDR)
    conv = ah.struct_of("md_conv_bwd_attrs", HDR, known={"md_conv_bwd_block": block})
    data = ah.struct_of("md_conv1x1_bwd_data_attrs", HDR)
    assert C.sizeof(block) == 16 and C.sizeof(conv) == 24 * 4 and C.sizeof(data) == 6 * 4

    for got, want in ((det_ops._ConvBwdBlock, block), (Block, block), (det_ops._ConvBwdAttrs, conv), (ConvBwd, conv),
                      (det_ops._Conv1x1BwdDataAttrs, data), (Conv1x1BwdData, data)):
        assert ah.same_layout(got, want), got
    at = det_ops.conv_bwd_attrs(64, 9, 4, 3, kernel=3, korder=1, blocks=[(0, 5, 0, 8), (5, 2, 8, 8)])
    assert [getattr(at, n) for n in ("cin", "cout", "x_c_off", "dy_c_off", "kernel", "korder", "n_blocks", "reserved0")] == [64, 9, 4, 3, 3, 1, 2, 0]
    assert [(b.row0, b.rows, b.col0, b.cols) for b in at.blocks] == [(0, 5, 0, 8), (5, 2, 8, 8), (0, 0, 0, 0), (0, 0, 0, 0)]
    with pytest.raises(ValueError):
        det_ops.conv_bwd_attrs(8, 8, blocks=[(0, 1, 0, 8)] * 5)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_convbwd", case)


def _block(k, *vals):
    def edit(c):
        c.extra.blocks[k] = Block(*vals)
    return edit


@pytest.mark.parametrize("tag", ["[pool, k3]", "[workspace, k3]", "[workspace, k1]", "[pool, k3, one block]"])
def test_wgrad_semantic_refusals_return_the_documented_codes(tag):
    case = _case(tag, "md_conv_bwd_weight")
    k = case.extra.kernel
    edits = [
        attr("reserved0", 1), attr("reserved0", -1), attr("cin", 0), attr("cin", -8), attr("cout", 0), attr("cout", -1),
        attr("x_c_off", -8), attr("dy_c_off", -1),
        attr("x_c_off", 16), attr("cin", 24), attr("dy_c_off", 6), attr("cout", 7),            # a channel range outside x / dy
        attr("kernel", 0), attr("kernel", 2), attr("kernel", 5), attr("kernel", -3), attr("korder", 2), attr("korder", -1),
        attr("n_blocks", -1), attr("n_blocks", 5),
        shape(0, (0, 3, 5, 16), B16), shape(0, (1, 0, 5, 16), B16), shape(1, (1, 3, 0, 8)),     # no pixel
        shape(1, (1, 3, 4, 8)), shape(1, (2, 3, 5, 8)), shape(0, (1, 5, 3, 16), B16),           # x and dy over different pixels
        shape(2, (2, 128)), shape(2, (32, k * k * 8 - 1)), shape(3, (2,)),                      # dw / db smaller than the layer
    ]
    # a block outside [0, cout) x [0, cin), or empty
    for vals in ((0, 4, 0, 8), (2, 2, 0, 8), (-1, 2, 0, 8), (0, 3, 1, 8), (0, 3, -1, 4), (0, 0, 0, 8), (0, 3, 0, 0), (3, 1, 0, 8), (0, 1, 8, 1)):
        edits.append(both(attr("n_blocks", 1), _block(0, *vals)))
    edits.append(both(attr("n_blocks", 2), _block(0, 0, 3, 0, 8), _block(1, 0, 4, 0, 8)))         # the second one
    for i, e in enumerate(edits):
        assert rc(case, e) == ARG, i
    for o, kk in ((2, 0), (2, 1), (3, 0), (3, 1), (3, 2)):                                         # an output at another operand's address
        assert raw(case, same=[(o, kk)]) == ARG, (o, kk)
    # the stated limits: each edit keeps every extent consistent, so the limit alone refuses it
    wide_x = both(shape(0, (1, 3, 5, 24), B16), attr("x_c_off", 0), shape(2, (32, 128)))
    assert rc(case, both(wide_x, attr("cin", 12))) == SIZE                                      # cin % 8
    many = both(shape(1, (1, 3, 5, 264)), shape(2, (264, 128)), shape(3, (264,)), attr("dy_c_off", 0))
    assert rc(case, both(many, attr("cout", 257))) == SIZE
    lim = 1024 if k == 1 else 256
    wide = both(shape(0, (1, 3, 5, lim + 16), B16), shape(2, (32, k * k * (lim + 8))), attr("x_c_off", 0))
    assert rc(case, both(wide, attr("cin", lim + 8))) == SIZE
    assert rc(case, attr("korder", 1)) == SIZE                                                   # korder 1 with cin 8
    huge = both(shape(0, (2 ** 16, 2 ** 15, 1, 16), B16), shape(1, (2 ** 16, 2 ** 15, 1, 8)))   # P = 2^31
    assert raw(case, huge) == SIZE
    assert raw(case, shape(0, (2 ** 16, 2 ** 15, 1, 16), B16)) == ARG                            # (dy no longer matches)
    assert raw(case, shape(2, (2 ** 16, 2 ** 15))) == SIZE                                       # dw of 2^31 elements
    if "workspace" in tag:
        assert rc(case, shape(4, (workspace_bytes(k) - 1,), U8)) == SIZE                         # one byte short


def test_a_misaligned_workspace_is_refused():
    """a workspace that is large enough and 8 bytes off a 16-byte boundary: rc 2, before any device call"""
    case = _case("[workspace, k3]", "md_conv_bwd_weight")
    call = edited(case, lambda c: None)
    n = call.n
    arena = (C.c_char * (4096 * (n + 2)))()
    base = (C.addressof(arena) + 4095) // 4096 * 4096
    params, ndims = (C.c_void_p * n)(), (C.c_int * n)()
    shapes, dtypes = (C.POINTER(C.c_int64) * n)(), (C.c_char_p * n)()
    keep = []
    for i, op in enumerate(case.operands):
        params[i] = base + 4096 * i + (8 if i == 4 else 0)                                         # the workspace 8 bytes off a 16-byte boundary
        keep.append((C.c_int64 * len(op.shape))(*op.shape))
        ndims[i], shapes[i], dtypes[i] = len(op.shape), C.cast(keep[-1], C.POINTER(C.c_int64)), op.dtype.encode()
    assert lib_handle().md_conv_bwd_weight(n, params, ndims, shapes, dtypes, None, C.byref(case.extra)) == ARG


@pytest.mark.parametrize("tag", ["[act]", "[no act]"])
def test_dgrad_semantic_refusals_return_the_documented_codes(tag):
    case = _case(tag, "md_conv1x1_bwd_data")
    act = tag == "[act]"
    edits = [
        attr("reserved0", 1), attr("cin", 0), attr("cin", -8), attr("cout", 0), attr("cout", -1), attr("dy_c_off", -1), attr("dx_c_off", -4),
        attr("act_c_off", -1),
        attr("dy_c_off", 6), attr("cout", 7), attr("dx_c_off", 5), attr("cin", 16),            # a channel range outside dy / dx
        shape(0, (0, 3, 5, 8)), shape(0, (1, 3, 0, 8)), shape(3, (1, 3, 4, 12)), shape(3, (2, 3, 5, 12)),
        shape(1, (2, 64), B16), shape(1, (32, 7), B16),                                          # w smaller than the layer
    ]
    edits += [attr("act_c_off", 5), shape(2, (1, 3, 4, 12), B16), shape(2, (1, 3, 5, 11), B16)] if act else [attr("act_c_off", 4)]
    for i, e in enumerate(edits):
        assert rc(case, e) == ARG, i
    for k in (0, 1) + ((2,) if act else ()):                                                       # dx at another operand's address
        assert raw(case, same=[(3, k)]) == ARG, k
    grow = lambda cin: both(shape(1, (32, cin + 8), B16), shape(3, (1, 3, 5, cin + 8)), shape(2, (1, 3, 5, cin + 8), B16) if act else (lambda c: None),
                             attr("dx_c_off", 0), attr("act_c_off", 0))
    assert rc(case, both(grow(16), attr("cin", 12))) == SIZE
    assert rc(case, both(grow(1040), attr("cin", 1032))) == SIZE
    assert rc(case, both(shape(0, (1, 3, 5, 264)), shape(1, (264, 64), B16), attr("dy_c_off", 0), attr("cout", 257))) == SIZE
    huge = both(shape(0, (2 ** 16, 2 ** 15, 1, 8)), shape(3, (2 ** 16, 2 ** 15, 1, 12)), shape(2, (2 ** 16, 2 ** 15, 1, 12), B16) if act else (lambda c: None))
    assert raw(case, huge) == SIZE
    big = both(shape(0, (2 ** 14, 2 ** 14, 1, 8)), shape(3, (2 ** 14, 2 ** 14, 1, 12)), shape(2, (2 ** 14, 2 ** 14, 1, 12), B16) if act else (lambda c: None))
    assert raw(case, big) == SIZE                                                                 # P = 2^28, dy of 2^31 elements


# ---------------------------------------------------------------------------------------------------- the judges against autograd
def _autograd(x, dy, w, b, k):
    """torch float64: x [N,H,W,cin], dy [N,H,W,cout], w [cout,cin,k,k] -> (dw, db, dx) of sum(conv2d(x, w, b) dy)"""
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wt = torch.from_numpy(w).requires_grad_(True)
    bt = torch.from_numpy(b).requires_grad_(True)
    y = torch.nn.functional.conv2d(xt, wt, bt, stride=1, padding=(k - 1) // 2)
    (y * torch.from_numpy(dy).permute(0, 3, 1, 2)).sum().backward()
    return wt.grad.numpy(), bt.grad.numpy(), xt.grad.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("k,korder,cin", [(1, 0, 16), (3, 0, 16), (3, 1, 64), (3, 0, 64)])
def test_wgrad_judge_equals_float64_autograd(k, korder, cin):
    rng = np.random.default_rng([k, korder, cin])
    N, H, W, cout, x_off, dy_off = 3, 5, 7, 6, 8, 2
    x, dy = rng.normal(0, 1, (N, H, W, cin + x_off + 3)), rng.normal(0, 1, (N, H, W, cout + dy_off + 1))
    w, b = rng.normal(0, 1, (cout, cin, k, k)), rng.normal(0, 1, cout)
    dw, db, _ = _autograd(np.ascontiguousarray(x[..., x_off:x_off + cin]), np.ascontiguousarray(dy[..., dy_off:dy_off + cout]), w, b, k)
    got = cc.wgrad_kxk(x, dy, cin, cout, kernel=k, korder=korder, x_c_off=x_off, dy_c_off=dy_off, rows=8, kpad=k * k * cin + 5)
    col = cc.columns(k, cin, korder)
    want = np.zeros((8, k * k * cin + 5))
    for t in range(k * k):
        want[:cout, col[t]] = dw[:, :, t // k, t % k]
    assert np.abs(got["dw"] - want).max() <= 1e-12 * np.abs(want).max() and np.abs(got["db"][:cout] - db).max() <= 1e-12 * np.abs(db).max()
    assert not got["dw"][cout:].any() and not got["dw"][:, k * k * cin:].any() and not got["db"][cout:].any()
    assert got["live"].sum() == cout * k * k * cin and (got["absdw"] >= np.abs(got["dw"]) * (1 - 1e-12)).all()
    # the block mask: the same numbers inside the blocks, zero outside, db dense
    blocks = [(0, 4, 0, 8), (4, 2, 8, cin - 8)]
    masked = cc.wgrad_kxk(x, dy, cin, cout, kernel=k, korder=korder, x_c_off=x_off, dy_c_off=dy_off, blocks=blocks, rows=8, kpad=k * k * cin + 5)
    inside = np.zeros((8, k * k * cin + 5), bool)
    for r0, nr, c0, nc in blocks:
        for t in range(k * k):
            inside[r0:r0 + nr, col[t][c0:c0 + nc]] = True
    assert np.array_equal(masked["live"], inside) and np.array_equal(masked["dw"], np.where(inside, got["dw"], 0.0))
    assert np.array_equal(masked["db"], got["db"]) and not masked["absdw"][~inside].any()


def test_wgrad_judge_with_kernel_1_is_the_pointwise_judge():
    s = dict(cin=40, cout=20, x_c_off=8, dy_c_off=0)
    rng = np.random.default_rng(5)
    x, dy = rng.normal(0, 1, (2, 5, 7, 48)).astype(np.float32), rng.normal(0, 1, (2, 5, 7, 24)).astype(np.float32)
    a, b = tc.wgrad(x, dy, rows=32, kpad=64, **s), cc.wgrad_kxk(x, dy, kernel=1, rows=32, kpad=64, **s)
    assert all(np.array_equal(a[k], b[k]) for k in ("dw", "db", "absdw", "absdb"))


def test_dgrad_judge_equals_float64_autograd():
    rng = np.random.default_rng(9)
    N, H, W, cin, cout = 3, 4, 5, 16, 6
    dy, w = rng.normal(0, 1, (N, H, W, cout + 3)), rng.normal(0, 1, (8, 24))
    pre = rng.normal(0, 1, (N, H, W, cin))                                           # the input of the ReLU whose output the layer reads
    xr = np.maximum(pre, 0.0)
    _, _, dx = _autograd(xr, np.ascontiguousarray(dy[..., 2:2 + cout]), np.ascontiguousarray(w[:cout, :cin]).reshape(cout, cin, 1, 1), np.zeros(cout), 1)
    got = cc.dgrad_1x1(dy, w, cin, cout, dy_c_off=2)
    assert np.abs(got["dx"] - dx).max() <= 1e-12 * np.abs(dx).max() and got["keep"].all()
    # through the ReLU: autograd of relu(pre) gives dx where pre > 0
    pt = torch.from_numpy(pre).requires_grad_(True)
    y = torch.relu(pt) @ torch.from_numpy(np.ascontiguousarray(w[:cout, :cin])).T
    (y * torch.from_numpy(np.ascontiguousarray(dy[..., 2:2 + cout]))).sum().backward()
    act = np.concatenate([np.zeros((N, H, W, 4)), xr], -1).astype(np.float32)
    masked = cc.dgrad_1x1(dy, w, cin, cout, act=act, dy_c_off=2, act_c_off=4)
    assert np.abs(masked["dx"] - pt.grad.numpy()).max() <= 1e-12 * np.abs(dx).max() and 0.3 < masked["keep"].mean() < 0.7
    # the mask's edge values
    edge = np.array([0.0, -0.0, -1.0, np.nan, 9.2e-41, 1.0, np.inf, -np.inf], np.float32).reshape(1, 1, 1, 8)
    k = cc.dgrad_1x1(np.ones((1, 1, 1, 1)), np.ones((1, 8)), 8, 1, act=edge)
    assert k["keep"].reshape(-1).tolist() == [False, False, False, False, True, True, True, False]
    assert cc.dgrad_chain_length(84) == 84 and np.array_equal(cc.dgrad_bound(4, np.ones(3)), np.full(3, 4 * 2.0 ** -24))


@pytest.mark.parametrize("korder", [0, 1])
def test_column_map_is_the_pack_order_of_pack_conv(korder):
    cin, cout = 128, 5
    w = torch.arange(cout * cin * 9, dtype=torch.float32).reshape(cout, cin, 3, 3) % 251          # bf16-exact integers
    pc = nn_ops.pack_conv(w, pad=1, korder=korder)
    assert pc.korder == korder and pc.cin == cin and tuple(pc.w.shape)[1] == 9 * cin
    col = cc.columns(3, cin, korder)
    packed = pc.w.float().numpy()
    for t in range(9):
        assert np.array_equal(packed[:cout, col[t]], w[:, :, t // 3, t % 3].numpy()), t
    assert np.array_equal(optim.pack_columns(pc).numpy(), col)
    assert sorted(col.reshape(-1).tolist()) == list(range(9 * cin))


# ---------------------------------------------------------------------------------------------------- schedule and configs
def test_multi_epochs_decay_lr_by_hand():
    lr = optim.multi_epochs_decay_lr(5e-4, [90, 120], steps_per_epoch=3, factor=10, total_step=3 * 140)
    assert len(lr) == 420 and lr[0] == lr[269] == 5e-4 and lr[270] == lr[359] == 5e-4 / 10 and lr[360] == lr[-1] == 5e-4 / 100
    assert optim.multi_epochs_decay_lr(1.0, (1, 1, 2), 2, 2, 6) == [1.0, 1.0, 0.25, 0.25, 0.125, 0.125]
    assert optim.multi_epochs_decay_lr(1.0, [], 5, 10, 3) == [1.0, 1.0, 1.0]
    with pytest.raises(TypeError):
        optim.multi_epochs_decay_lr(1.0, 90, 5, 10, 3)
    with pytest.raises(ValueError):
        optim.multi_epochs_decay_lr(1.0, [1], 0, 10, 3)
    assert "utils.py:501-538" in optim.multi_epochs_decay_lr.__doc__


@pytest.mark.parametrize("name", ["r18_dcn", "tiny"])
def test_train_configs_carry_the_optimizer_and_the_schedule(name):
    from minddet.models import Config

    t = Config.fromfile(os.path.join(ROOT, "configs", "centernet", f"centernet_{name}_train.py")).train_cfg
    assert t["optimizer"] == dict(type="Adam", eps=1e-7, weight_decay=0.0)
    assert t["lr_config"] == dict(type="MultiEpochsDecayLR", learning_rate=5e-4, multi_epochs=[90, 120], factor=10, warmup_steps=0, batch_size=16)
    assert set(t["optimizer"]) - {"type"} <= set(optim.CENTERNET_OPTIMIZER) and optim.CENTERNET_OPTIMIZER["grad_scale"] == 1.0
    c = t["lr_config"]
    lr = optim.multi_epochs_decay_lr(c["learning_rate"], c["multi_epochs"], 2, c["factor"], 2 * 140)
    assert (lr[179], lr[180], lr[240]) == (5e-4, 5e-4 / 10, 5e-4 / 100)


def test_the_trainer_refuses_what_is_not_built():
    class Stub:
        pass

    for cfg in (dict(type="SGD"), dict(type="Adam", momentum=0.9), dict(type="Adam", max_norm=35.0)):
        with pytest.raises(ValueError):
            optim.CenterNetHeadTrainer(Stub(), cfg)
