"""CPU: the KITTI PointPillars training loss without a GPU -- the ABI of include/minddet_hip_pploss.h (the two functions exported,
the semantic refusals answered before any device call, the ctypes mirrors laid out as the header says), the
contract tests/pp_loss_contract.py against a literal torch-float64 transcription of the reference's losses.py and
pointpillars.py:19-127, 817-872 under autograd on the reference's own assigner outputs (tests/golden/target_vectors.npz), and the
train configs.

Criteria of the comparison, fixed beforehand: losses to 1e-12 relative; the structural zeros of the gradient exact on both sides; every
other gradient element, rounded to fp32, differs in at most 1 in 10^4, by 1 ulp.  Measured: 0 differing of the 4 710 / 13 662 / 163
cls elements and 0 of the box / dir elements, relative loss differences <= 4e-16."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F_

from minddet_amd import det_ops
from tests import pp_loss_contract as pl
from tests import abi_header as ah
from tests.abi_cases import B16, I, U8
from tests.abi_cases_pploss import CASES, PPLoss
from tests.abi_derive import attr, both, item, lib_handle, rc, refuse_single_defects, shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = ah.header("minddet_hip_pploss.h")
HDR_PP = ah.header("minddet_hip_pp.h")
G = np.load(os.path.join(ROOT, "tests", "golden", "target_vectors.npz"))
# fixture -> (H, W, A, K): N = H W A
FIXTURE_SHAPES = dict(car=(54, 62, 2, 1), pedcyc=(40, 60, 4, 2), nogt=(10, 12, 2, 1))


def test_header_declares_the_two_symbols_and_the_library_exports_them():
    assert ah.aot_symbols(HDR) == ["md_pp_loss", "md_pp_loss_grad"] and '#include "minddet_hip_pp.h"' in HDR
    assert "pointpillars.py:817-872" in HDR and "losses.py:40-191" in HDR
    assert "minddet_hip_pploss.h" in open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    assert {c.sym for c in CASES} == {"md_pp_loss", "md_pp_loss_grad"} and len({c.id for c in CASES}) == len(CASES)
    lib = lib_handle()
    for sym in ("md_pp_loss", "md_pp_loss_grad"):
        assert getattr(lib, sym)(0, None, None, None, None, None, None) == 1             # wrong parameter count, before anything else


def test_ctypes_mirrors_have_the_headers_layout():
    head = ah.struct_of("md_pp_head_attrs", HDR_PP)
    want = ah.struct_of("md_pp_loss_attrs", HDR, known={"md_pp_head_attrs": head})
    assert C.sizeof(head) == 7 * 4 and C.sizeof(want) == 28 + 12 + 28 + 12 + 8

    for got in (det_ops._PPLossAttrs, PPLoss):
        assert ah.same_layout(got, want), got
    for got in (det_ops._PPHeadAttrs, dict(PPLoss._fields_)["head"]):
        assert ah.layout(got) == ah.layout(head), got
    defines = ah.defines(HDR)
    assert defines["MD_PP_LOSS_STRIP"] == 64 and defines["MD_PP_LOSS_COUNT_CHUNK"] == 4096
    # (each decides the library's answer: 64 cells are one strip of 40 bytes, 4096 labels one count of 4)
    assert [det_ops.pp_loss_workspace_bytes(1, 1, w, 1) for w in (64, 65)] == [40 + 4, 80 + 4]
    assert [det_ops.pp_loss_workspace_bytes(1, 64, 64, a) for a in (1, 2)] == [40 * 64 + 4, 40 * 64 + 8]
    assert defines["MD_PP_LOSS_MAX_CHANNELS"] >= 2 * 48                                   # both shipped heads (C = 24, 48) with room to spare


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_pploss", case)


@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=[CASES[0].id, CASES[3].id])
def test_semantic_refusals_return_the_documented_codes(case):
    ARG, SIZE = 2, 4
    grad = case.sym == "md_pp_loss_grad"

    def head(name, value):
        return lambda c: setattr(c.extra.head, name, value)

    nan, inf = float("nan"), float("inf")
    edits = [
        head("num_anchors", 0), head("num_anchors", -1), head("num_classes", 0), head("num_anchors", 3), head("num_classes", 2),  # N / channels
        head("off_cls", -1), head("off_cls", 23), head("off_box", 11), head("off_box", -1), head("off_dir", 21),                # outside [0, C)
        head("off_dir", -2),
        head("off_box", 1), head("off_dir", 15), head("off_cls", 15), head("off_dir", 0),                                        # two heads on a channel
        head("score_mode", 1), head("self_train", 0),
        attr("gamma", -0.5), attr("sigma", 0.0), attr("sigma", -3.0), attr("pos_cls_weight", 0.0), attr("neg_cls_weight", 0.0),
        attr("pos_cls_weight", -1.0), attr("neg_cls_weight", -1.0),
        attr("alpha", nan), attr("alpha", -inf), attr("gamma", inf), attr("gamma", nan), attr("sigma", inf), attr("sigma", nan),
        attr("cls_weight", nan), attr("loc_weight", inf), attr("dir_weight", -inf), attr("pos_cls_weight", inf), attr("neg_cls_weight", nan),
        item("code_weights", 0, nan), item("code_weights", 6, -inf),
        shape(0, (0, 8, 12, 24), B16),                                                        # an empty batch
        shape(0, (1, 0, 12, 24), B16), shape(0, (1, 8, 0, 24), B16),
        shape(0, (2, 8, 12, 24), B16), shape(0, (1, 8, 11, 24), B16), shape(1, (1, 191), I), shape(1, (2, 192), I), shape(2, (1, 192, 6)),
        shape(2, (1, 191, 7)), shape(2, (2, 192, 7)), shape(3, (191, 7)), shape(3, (192, 6)), shape(3, (192, 8)), shape(4, (4,)),
        shape(4, (6,)), shape(5, (2,)), shape(6, (2,)),
    ]
    if grad:
        edits += [shape(7, (1, 8, 12, 16)), shape(7, (1, 12, 8, 24)), shape(7, (2, 8, 12, 24))]
    for i, e in enumerate(edits):
        assert rc(case, e) == ARG, i
    wide = both(shape(0, (1, 8, 12, 136), B16), *([shape(7, (1, 8, 12, 136))] if grad else []))   # C above the LDS bound
    assert rc(case, wide) == SIZE
    many = both(shape(0, (65536, 1, 1, 24), B16), shape(1, (65536, 2), I), shape(2, (65536, 2, 7)), shape(3, (2, 7)), shape(5, (65536,)),
                *([shape(7, (65536, 1, 1, 24))] if grad else []))                                 # B above the grid bound
    assert rc(case, many) == SIZE
    if "[workspace]" in case.id:
        assert rc(case, shape(len(case.operands) - 1, (83,), U8)) == SIZE                    # one byte short of 40 B strips + 4 B chunks


# ---------------------------------------------------------------------------------------------------- the reference, transcribed
def clip_by_value(x, lo, hi):
    """MindSpore's clip_by_value as its composite form evaluates it: the upper bound first, then the lower (so the lower bound wins
    when they cross, which is what keeps the normaliser at 1 when no sample has a positive).  The derivative passes on the bounds
    themselves (torch.clamp), so that the many logits equal to logits.max() keep theirs."""
    return torch.clamp(torch.clamp(x, max=float(hi)), min=float(lo))


def prepare_loss_weights(labels, pos_cls_weight, neg_cls_weight, dtype):
    """pointpillars.py:19-43"""
    cared = labels >= 0
    positives = labels > 0
    negatives = labels == 0
    negative_cls_weights = negatives.to(dtype) * neg_cls_weight
    cls_weights = negative_cls_weights + pos_cls_weight * positives.to(dtype)
    reg_weights = positives.to(dtype)
    pos_normalizer = positives.to(dtype).sum(1, keepdim=True)              # (float16 in the reference: exact up to 2048 positives)
    one = 1.0
    reg_weights = reg_weights / clip_by_value(pos_normalizer, one, pos_normalizer.max())
    cls_weights = cls_weights / clip_by_value(pos_normalizer, one, pos_normalizer.max())
    return cls_weights, reg_weights, cared


def one_hot(indices, depth, dtype):
    """ops.OneHot: an index outside [0, depth) gives an all-zero row"""
    return (indices.unsqueeze(-1) == torch.arange(depth)).to(dtype)


def sigmoid_cross_entropy_with_logits(logits, labels):
    """losses.py:40-46"""
    loss = clip_by_value(logits, 0.0, logits.max().detach()) - logits * labels.to(logits.dtype)
    loss = loss + torch.log1p(torch.exp(-torch.abs(logits)))
    return loss


def sigmoid_focal_loss(prediction_tensor, target_tensor, weights, gamma, alpha, sigmoid_form=False):
    """SigmoidFocalClassificationLoss.construct, losses.py:71-99; sigmoid_form: 1 - p_t written as the sigmoid of the signed logit
    (the same real function, without the subtraction that loses every digit beyond |x| ~ 37)"""
    weights = weights.unsqueeze(2)
    per_entry_cross_ent = sigmoid_cross_entropy_with_logits(labels=target_tensor, logits=prediction_tensor)
    if sigmoid_form:
        one_minus_pt = target_tensor * torch.sigmoid(-prediction_tensor) + (1 - target_tensor) * torch.sigmoid(prediction_tensor)
    else:
        prediction_probabilities = torch.sigmoid(prediction_tensor)
        p_t = (target_tensor * prediction_probabilities) + ((1 - target_tensor) * (1 - prediction_probabilities))
        one_minus_pt = 1.0 - p_t
    modulating_factor = 1.0
    if gamma:
        modulating_factor = torch.pow(one_minus_pt, gamma)
    alpha_weight_factor = 1.0
    if alpha is not None:
        alpha_weight_factor = target_tensor * alpha + (1 - target_tensor) * (1 - alpha)
    focal_cross_entropy_loss = modulating_factor * alpha_weight_factor * per_entry_cross_ent
    return focal_cross_entropy_loss * weights


def smooth_l1_loss(prediction_tensor, target_tensor, weights, sigma, code_weights):
    """WeightedSmoothL1LocalizationLoss.construct, losses.py:121-154 (codewise)"""
    diff = prediction_tensor - target_tensor
    diff = code_weights.view(1, 1, -1) * diff
    abs_diff = torch.abs(diff)
    abs_diff_lt_1 = (abs_diff <= 1 / (sigma ** 2)).to(abs_diff.dtype)
    loss = abs_diff_lt_1 * 0.5 * torch.pow(abs_diff * sigma, 2) + (abs_diff - 1 / (2 * (sigma ** 2))) * (1.0 - abs_diff_lt_1)
    return loss * weights.unsqueeze(-1)


def softmax_loss(prediction_tensor, target_tensor, weights):
    """WeightedSoftmaxClassificationLoss.construct, losses.py:171-191"""
    num_classes = prediction_tensor.shape[-1]
    per_row = F_.cross_entropy(prediction_tensor.reshape(-1, num_classes), target_tensor.reshape(-1, num_classes).argmax(-1), reduction="none")
    return per_row.view(weights.shape) * weights


def add_sin_difference(boxes1, boxes2):
    """pointpillars.py:101-107"""
    rad_pred_encoding = torch.sin(boxes1[..., -1:]) * torch.cos(boxes2[..., -1:])
    rad_tg_encoding = torch.cos(boxes1[..., -1:]) * torch.sin(boxes2[..., -1:])
    return torch.cat([boxes1[..., :-1], rad_pred_encoding], -1), torch.cat([boxes2[..., :-1], rad_tg_encoding], -1)


def get_pos_neg_loss(cls_loss, labels):
    """pointpillars.py:110-127"""
    batch_size = cls_loss.shape[0]
    if cls_loss.shape[-1] == 1 or len(cls_loss.shape) == 2:
        cls_pos_loss = ((labels > 0).to(cls_loss.dtype) * cls_loss.view(batch_size, -1)).sum() / batch_size
        cls_neg_loss = ((labels == 0).to(cls_loss.dtype) * cls_loss.view(batch_size, -1)).sum() / batch_size
    else:
        cls_pos_loss = cls_loss[..., 1:].sum() / batch_size
        cls_neg_loss = cls_loss[..., 0].sum() / batch_size
    return cls_pos_loss, cls_neg_loss


def loss_cell(head, labels, reg_targets, anchors, *, off_cls, off_box, off_dir, num_anchors, num_classes, alpha=0.25, gamma=2.0, sigma=3.0,
              code_weights=(1.0,) * 7, cls_weight=1.0, loc_weight=2.0, dir_weight=0.2, pos_cls_weight=1.0, neg_cls_weight=1.0,
              sigmoid_form=False):
    """PointPillarsWithLossCell.construct, pointpillars.py:817-872, on float64: head [B,H,W,C] (requires_grad) is cut into the network's
    three outputs; labels / reg_targets / anchors numpy -> (total, (loc, cls, dir, cls_pos, cls_neg))"""
    B = head.shape[0]
    A, K, dt = num_anchors, num_classes, head.dtype
    f = pl.f32
    cls_preds = head[..., off_cls:off_cls + A * K].reshape(B, -1, K)
    box_preds = head[..., off_box:off_box + A * 7].reshape(B, -1, 7)
    lab = torch.from_numpy(labels.astype(np.int64))
    tg = torch.from_numpy(reg_targets).to(dt)
    loss, dir_part = 0, torch.tensor(0.0, dtype=dt)
    if off_dir is not None:
        rot_gt = torch.from_numpy(reg_targets[..., -1] + anchors[None, :, -1])                # fp32, as the reference's tensors are
        dir_targets = one_hot((rot_gt > 0).long(), 2, dt)
        dir_logits = head[..., off_dir:off_dir + A * 2].reshape(B, -1, 2)
        weights = (lab > 0).to(dt)
        wsum = weights.sum(-1, keepdim=True)
        weights = weights / clip_by_value(wsum, 1.0, wsum.max())
        dir_loss = softmax_loss(dir_logits, dir_targets, weights).sum() / B
        dir_part = dir_loss * f(dir_weight)
        loss = dir_part
    cls_weights, reg_weights, cared = prepare_loss_weights(lab, f(pos_cls_weight), f(neg_cls_weight), dt)
    cls_targets = lab * cared.to(lab.dtype)
    one_hot_targets = one_hot(cls_targets, K + 1, dt)[..., 1:]
    bp, rt = add_sin_difference(box_preds, tg)
    cwt = torch.tensor([f(v) for v in code_weights], dtype=dt)
    loc_loss = smooth_l1_loss(bp, rt, reg_weights, f(sigma), cwt)
    cls_loss = sigmoid_focal_loss(cls_preds, one_hot_targets, cls_weights, f(gamma), None if alpha is None else f(alpha), sigmoid_form)
    loc_loss_reduced = loc_loss.sum() / B * f(loc_weight)
    cls_pos_loss, cls_neg_loss = get_pos_neg_loss(cls_loss, lab)
    cls_pos_loss = cls_pos_loss / f(pos_cls_weight)
    cls_neg_loss = cls_neg_loss / f(neg_cls_weight)
    cls_loss_reduced = cls_loss.sum() / B * f(cls_weight)
    loss = loss + (loc_loss_reduced + cls_loss_reduced)
    return loss, (loc_loss_reduced, cls_loss_reduced, dir_part, cls_pos_loss, cls_neg_loss)


# ---------------------------------------------------------------------------------------------------- data
def bf16(x):
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def layout(A, K, order=("cls", "box", "dir"), C=None, direction=True):
    """the three heads side by side in `order` -> (dict(off_cls, off_box, off_dir, num_anchors, num_classes), C rounded up to 8)"""
    width, off, base = dict(cls=A * K, box=A * 7, dir=A * 2), dict(off_dir=None), 0
    for h in order:
        if h == "dir" and not direction:
            continue
        off["off_" + h] = base
        base += width[h]
    return dict(off, num_anchors=A, num_classes=K), (base + 7) // 8 * 8 if C is None else C


def fixture(name):
    """-> labels [1,N] i32, reg_targets [1,N,7] f32, anchors [N,7] f32 of the reference's assigner (tests/golden/target_vectors.npz)"""
    return G[name + "_labels"][None].astype(np.int32), G[name + "_targets"][None].astype(np.float32), G[name + "_anchors"].astype(np.float32)


def predictions(rng, shape, lay, cls_limit=12.0, uniform=False):
    """seeded head values as the fp32 values of bf16 numbers: N(0, 1.5) on the box and direction channels, cls logits N(0, 4) cut to
    +-cls_limit (uniform: spread evenly over that range); no cls logit is exactly 0 (the transcription's |x| has no derivative there)"""
    head = rng.normal(0, 1.5, shape).astype(np.float32)
    c0, n = lay["off_cls"], lay["num_anchors"] * lay["num_classes"]
    cls_shape = shape[:3] + (n,)
    x = rng.uniform(-cls_limit, cls_limit, cls_shape) if uniform else np.clip(rng.normal(0, 4.0, cls_shape), -cls_limit, cls_limit)
    head[..., c0:c0 + n] = np.where(x == 0, 0.5, x)
    head = bf16(head)
    assert np.abs(head[..., c0:c0 + n]).max() <= cls_limit and (head[..., c0:c0 + n] != 0).all()
    return head


def compare_with_transcription(tag, head, labels, reg, anchors, lay, settings, sigmoid_form=False, min_nonzero=1):
    want = pl.loss(head, labels, reg, anchors, **lay, **settings)
    h64 = torch.from_numpy(head).to(torch.float64).requires_grad_(True)
    total, parts = loss_cell(h64, labels, reg, anchors, **lay, **settings, sigmoid_form=sigmoid_form)
    (g,) = torch.autograd.grad(total, h64)
    g = g.numpy()

    def rel(a, b):
        return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)

    worst = max([rel(want["total"], total.detach())] + [rel(want["parts"][i], parts[i].detach()) for i in range(5) if float(parts[i].detach()) != 0])
    assert all(want["parts"][i] == 0 for i in range(5) if float(parts[i].detach()) == 0)
    assert np.array_equal(want["num_pos"], (labels > 0).sum(1))
    counts = {}
    A, K = lay["num_anchors"], lay["num_classes"]
    groups = dict(cls=(lay["off_cls"], A * K), box=(lay["off_box"], A * 7))
    if lay["off_dir"] is not None:
        groups["dir"] = (lay["off_dir"], A * 2)
    for name, (c0, n) in groups.items():
        a, b, st = g[..., c0:c0 + n], want["grad"][..., c0:c0 + n], want["structural"][..., c0:c0 + n]
        assert not a[st].any() and not b[st].any(), name                                      # the structural zeros, exactly
        apart = pl.ulps_apart(a[~st].astype(np.float32), b[~st].astype(np.float32))
        counts[name] = (int((~st).sum()), int((apart > 0).sum()), int(apart.max()) if apart.size else 0)
    owned = np.zeros(head.shape[3], bool)
    for c0, n in groups.values():
        owned[c0:c0 + n] = True
    assert not g[..., ~owned].any() and not want["grad"][..., ~owned].any()
    assert not want["grad"][want["structural"]].any()
    print(f"pp_loss[{tag}]: total {float(total.detach()):.6f}, losses worst relative difference {worst:.2e}; per head (elements outside the structural zeros, differing "
          f"after rounding to fp32, worst ulp) {counts}")
    assert worst <= 1e-12
    for name, (nnz, ndiff, worst_ulp) in counts.items():
        assert worst_ulp <= 1 and ndiff * 10000 <= nnz, (name, nnz, ndiff, worst_ulp)
    assert counts["cls"][0] >= min_nonzero
    return want, counts


@pytest.mark.parametrize("name", ["car", "pedcyc", "nogt"])
def test_contract_equals_the_reference_transcription_under_autograd(name):
    H, W, A, K = FIXTURE_SHAPES[name]
    labels, reg, anchors = fixture(name)
    lay, C_ = layout(A, K)
    head = predictions(np.random.default_rng(7), (1, H, W, C_), lay)
    want, counts = compare_with_transcription(name, head, labels, reg, anchors, lay, dict(pl.DEFAULTS))
    cared = int((labels >= 0).sum())
    assert counts["cls"][0] == cared * K and cared == dict(car=4710, pedcyc=6831, nogt=163)[name]
    npos = int((labels > 0).sum())
    assert npos == dict(car=16, pedcyc=13, nogt=0)[name] and counts["box"][0] == 7 * npos and counts["dir"][0] == 2 * npos
    if name == "nogt":
        assert want["parts"][0] == 0 and want["parts"][2] == 0 and want["parts"][3] == 0 and want["parts"][1] > 0   # the clamp: n_b = 1


@pytest.mark.parametrize("name", ["car", "pedcyc"])
def test_contract_equals_the_sigmoid_form_out_to_40(name):
    """beyond +-12 the literal 1 - p loses digits; there the contract is held to the transcription whose 1 - p_t is sigmoid(s)"""
    H, W, A, K = FIXTURE_SHAPES[name]
    labels, reg, anchors = fixture(name)
    lay, C_ = layout(A, K)
    head = predictions(np.random.default_rng(40), (1, H, W, C_), lay, cls_limit=40.0, uniform=True)
    # the one place where the transcription itself loses digits: on a positive's own class autograd forms d ce / d x as 1 - 1 - e^-x
    # (the clip's 1, the label's -1, the log1p's share), which is exact to 1e-16 absolute only; those few logits stay below 12
    own = np.zeros((1, H * W * A, K), bool)
    for k in range(K):
        own[..., k] = labels == k + 1
    cls = head[..., lay["off_cls"]:lay["off_cls"] + A * K]
    cls[own.reshape(cls.shape) & (cls > 12)] = 12.0
    assert own.sum() == (labels > 0).sum() and (np.abs(cls) > 30).sum() > 1000
    compare_with_transcription(name + ", +-40", head, labels, reg, anchors, lay, dict(pl.DEFAULTS), sigmoid_form=True, min_nonzero=4000)


FURTHER = {
    "alpha None": dict(alpha=None),
    "gamma 0": dict(gamma=0.0),
    "gamma 1.5": dict(gamma=1.5),
    "weights": dict(code_weights=(1.0, 0.5, 2.0, 1.0, 0.25, 1.5, 0.75), cls_weight=1.5, loc_weight=0.75, dir_weight=0.4, pos_cls_weight=2.0,
                    neg_cls_weight=0.5, sigma=2.0),
}


@pytest.mark.parametrize("tag", list(FURTHER) + ["no direction head", "box dir cls order"])
def test_further_settings_equal_the_transcription(tag):
    H, W, A, K = FIXTURE_SHAPES["pedcyc"]
    labels, reg, anchors = fixture("pedcyc")
    lay, C_ = layout(A, K, direction=tag != "no direction head", order=("box", "dir", "cls") if tag == "box dir cls order" else ("cls", "box", "dir"))
    head = predictions(np.random.default_rng(3), (1, H, W, C_), lay)
    want, _ = compare_with_transcription(tag, head, labels, reg, anchors, lay, dict(pl.DEFAULTS, **FURTHER.get(tag, {})))
    if tag == "no direction head":
        assert want["parts"][2] == 0 and want["total"] == want["parts"][0] + want["parts"][1]


def test_planted_anchors_equal_the_transcription():
    """a label above K (a positive whose one-hot row is all zero), pred equal to target (gradient 0), a direction sum of exactly 0
    (bin 0), two samples of which one has no positive"""
    H, W, A, K = 3, 5, 2, 3
    N = H * W * A
    rng = np.random.default_rng(9)
    lay, C_ = layout(A, K, order=("box", "dir", "cls"))
    labels = np.zeros((2, N), np.int32)
    labels[0, [1, 4, 9, 17, 22, 29]] = [1, 2, 3, K + 2, 1, 3]
    labels[0, [2, 3, 11]] = -1
    labels[1, [0, 5]] = -1
    reg = np.zeros((2, N, 7), np.float32)
    reg[0] = bf16(rng.normal(0, 1, (N, 7)))
    anchors = np.zeros((N, 7), np.float32)
    anchors[:, 6] = np.tile([0.0, 1.57], N // 2)
    head = predictions(rng, (2, H, W, C_), lay)
    cells = head.reshape(2, H * W, C_)
    n = 4                                                                                     # pred equal to target on every code
    cells[0, n // A, lay["off_box"] + (n % A) * 7:lay["off_box"] + (n % A) * 7 + 7] = reg[0, n]
    n = 9                                                                                     # reg + anchor rotation == 0 exactly
    reg[0, n, 6] = -anchors[n, 6]
    n = 22
    reg[0, n, 6] = np.float32(-1e-3) - anchors[n, 6]
    want, counts = compare_with_transcription("planted", head, labels, reg, anchors, lay, dict(pl.DEFAULTS))
    g = want["grad"].reshape(2, H * W, C_)
    assert want["num_pos"].tolist() == [6.0, 0.0]
    assert not g[0, 2, lay["off_box"]:lay["off_box"] + 7].any() and not want["structural"].reshape(2, H * W, C_)[0, 2, lay["off_box"]:lay["off_box"] + 7].any()
    d9 = g[0, 9 // A, lay["off_dir"] + (9 % A) * 2:lay["off_dir"] + (9 % A) * 2 + 2]
    assert d9[0] < 0 < d9[1]                                                                  # bin 0 is the target: its logit is pushed up
    row = g[0, 17 // A, lay["off_cls"] + (17 % A) * K:lay["off_cls"] + (17 % A) * K + K]
    assert (row > 0).all()                                                                    # the label above K: every class is a negative ...
    assert g[0, 17 // A, lay["off_box"] + (17 % A) * 7:lay["off_box"] + (17 % A) * 7 + 7].any()   # ... on a positive anchor
    assert not g[1][:, lay["off_box"]:lay["off_cls"]].any() and counts["box"][0] == 7 * 6 and counts["dir"][0] == 12


# ---------------------------------------------------------------------------------------------------- configs
@pytest.mark.parametrize("name,A,K,thr", [("car", 2, 1, (0.6, 0.45)), ("ped_cycle", 4, 2, (0.5, 0.35))])
def test_train_configs_build_the_loss(name, A, K, thr):
    from minddet.models import Config
    from minddet_amd import graphs
    from minddet_amd.registry import build_detector

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", f"pointpillars_{name}_xyres16_train.py"))
    t = cfg.train_cfg
    assert t["loss"] == dict(classification_loss=dict(alpha=0.25, gamma=2.0),
                             localization_loss=dict(sigma=3.0, code_weight=[1.0] * 7), classification_weight=1.0, localization_weight=2.0)
    assert (t["direction_loss_weight"], t["pos_class_weight"], t["neg_class_weight"]) == (0.2, 1.0, 1.0)
    assert (t["assigner"]["matched_threshold"], t["assigner"]["unmatched_threshold"]) == thr
    assert all((g["matched_threshold"], g["unmatched_threshold"]) == thr for g in cfg.model["anchor_generators"])
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    assert isinstance(model, graphs.PointPillarsKITTIPoints) and model.inner.train_cfg == dict(t)
    loss = det_ops.PointPillarsLoss.from_config(cfg, model)
    at, off = loss.at, model.inner.head_offsets()
    assert (at.head.off_cls, at.head.off_box, at.head.off_dir, at.head.num_anchors, at.head.num_classes, at.head.score_mode, at.head.self_train) == \
        (off["cls"], off["box"], off["dir_cls"], A, K, 0, 1) == (0, A * K, A * K + 7 * A, A, K, 0, 1)
    assert [round(float(v), 6) for v in (at.alpha, at.gamma, at.sigma, at.cls_weight, at.loc_weight, at.dir_weight, at.pos_cls_weight, at.neg_cls_weight)] == \
        [0.25, 2.0, 3.0, 1.0, 2.0, 0.2, 1.0, 1.0] and list(at.code_weights) == [1.0] * 7
    same = model.inner.loss_op().at
    assert bytes(same) == bytes(at)
    fh, fw = model.inner.feature_hw
    assert det_ops.pp_loss_workspace_bytes(4, fh, fw, A) == 40 * 4 * ((fh * fw + 63) // 64) + 4 * 4 * ((fh * fw * A + 4095) // 4096)
    none = det_ops.PointPillarsLoss(off, A, K, dict(t["loss"], classification_loss=dict(alpha=None, gamma=0.0)))
    assert none.at.alpha < 0 and none.at.gamma == 0
    with pytest.raises(ValueError):
        det_ops.pp_loss_attrs(off, A, K, code_weights=[1.0] * 6)
