"""CPU: the CenterNet training loss without a GPU -- the ABI of include/minddet_hip_cn.h (the semantic
refusals answered before any device call), the contract tests/cn_loss_contract.py against a literal torch-float64 transcription of the
reference's Sigmoid / FocalLoss / RegLoss / CenterNetLossCell under autograd on the committed reference targets
(tests/golden/cn_target_vectors.npz), and the refusals of det_ops.CenterNetLoss."""
import numpy as np
import pytest
import torch

from minddet_amd import det_ops
from tests import cn_loss_contract as cl
from tests.abi_cases import B16, I, U8
from tests.abi_cases_cn import LOSS_CASES
from tests.abi_derive import attr, both, rc, refuse_single_defects, shape
from tests.test_cn_targets_cpu import fixture_case

WEIGHTS = dict(hm_weight=1.0, wh_weight=float(np.float32(0.1)), off_weight=1.0)      # the values an fp32 attribute struct carries


@pytest.mark.parametrize("case", LOSS_CASES, ids=[c.id for c in LOSS_CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_cn", case)


@pytest.mark.parametrize("case", [LOSS_CASES[0], LOSS_CASES[3]], ids=[LOSS_CASES[0].id, LOSS_CASES[3].id])
def test_semantic_refusals_return_the_documented_codes(case):
    ARG, SIZE = 2, 4
    grad = case.sym == "md_cn_loss_grad"
    nan, inf = float("nan"), float("inf")
    edits = [
        attr("num_classes", 2), attr("num_classes", 4), attr("num_classes", 0),               # num_classes != C
        attr("off_hm", -1), attr("off_hm", 6), attr("off_wh", 7), attr("off_wh", -1), attr("off_reg", 7), attr("off_reg", -2),
        attr("off_wh", 2), attr("off_reg", 4), attr("off_reg", 2), attr("off_hm", 1),         # two heads on one channel
        attr("hm_weight", nan), attr("wh_weight", inf), attr("off_weight", -inf),
        shape(0, (0, 8, 12, 8), B16),                                                         # an empty batch
        shape(0, (2, 8, 12, 8), B16), shape(1, (1, 3, 8, 11)), shape(1, (1, 3, 9, 12)), shape(1, (1, 2, 8, 12)), shape(1, (2, 3, 8, 12)),
        shape(2, (1, 5), I), shape(2, (2, 4), I), shape(3, (1, 3), U8), shape(4, (1, 4, 3)), shape(4, (1, 5, 2)), shape(5, (2, 4, 2)),
        shape(5, (1, 4, 1)), shape(6, (4,)), shape(6, (2,)), shape(7, (2,)), shape(8, (2,)),
    ]
    if grad:
        edits += [shape(9, (1, 8, 12, 16)), shape(9, (1, 12, 8, 8)), shape(9, (2, 8, 12, 8))]
    for i, e in enumerate(edits):
        assert rc(case, e) == ARG, i
    assert rc(case, attr("off_reg", -1)) is not None                                       # (no offset head: accepted, checked on the GPU)
    big = 1100                                                                                # M above the LDS bound
    grow = both(shape(2, (1, big), I), shape(3, (1, big), U8), shape(4, (1, big, 2)), shape(5, (1, big, 2)))
    assert rc(case, grow) == SIZE
    wide = both(shape(0, (1, 8, 12, 168), B16), *([shape(9, (1, 8, 12, 168))] if grad else []))   # Cp above the LDS bound
    assert rc(case, wide) == SIZE
    huge = both(shape(0, (1, 1 << 14, 1 << 13, 8), B16), shape(1, (1, 3, 1 << 14, 1 << 13)),      # operands of 2^30 elements and more
                *([shape(9, (1, 1 << 14, 1 << 13, 8))] if grad else []))
    assert rc(case, huge) == SIZE
    if "[workspace]" in case.id:
        assert rc(case, shape(len(case.operands) - 1, (67,), U8)) == SIZE                  # one byte short


# ---------------------------------------------------------------------------------------------------- the reference, transcribed
def sigmoid_cell(x):
    """Sigmoid.construct, utils.py:149-157"""
    return torch.clamp(torch.sigmoid(x), min=1e-4, max=1 - 1e-4)


def focal_loss(out, target, one_minus_out=None):
    """FocalLoss.construct, utils.py:187-207 (alpha 2, beta 4); one_minus_out: what stands for `1 - out` (None: the literal 1 - out)"""
    om = 1 - out if one_minus_out is None else one_minus_out
    pos_inds = (target == 1.0).to(out.dtype)
    neg_inds = (target < 1.0).to(out.dtype)
    neg_weights = torch.pow(1 - target, 4)
    pos_loss = torch.log(out) * torch.pow(om, 2) * pos_inds
    neg_loss = torch.log(om) * torch.pow(out, 2) * neg_weights * neg_inds
    num_pos = pos_inds.sum()
    num_pos = torch.where(num_pos == 0.0, torch.ones_like(num_pos), num_pos)
    return -(pos_loss.sum() + neg_loss.sum()) / num_pos


def reg_loss(output, mask, ind, target):
    """RegLoss.construct, utils.py:235-245, mode "l1" (nn.L1Loss(reduction="sum")) behind TransposeGatherFeature (:122-129)"""
    feat = output.permute(0, 2, 3, 1)
    feat = feat.reshape(feat.shape[0], -1, feat.shape[3])
    pred = feat.gather(1, ind.unsqueeze(2).expand(ind.shape[0], ind.shape[1], feat.shape[2]))
    mask = mask.to(output.dtype)
    num = mask.sum() * 2
    mask = mask.unsqueeze(2)
    return (pred * mask - target * mask).abs().sum() / (num + 1e-4)


def loss_cell(head, example, num_classes, off_hm, off_wh, off_reg, hm_weight, wh_weight, off_weight, negated_sigmoid=False):
    """CenterNetLossCell.construct, centernet_det.py:206-237, one stack, on float64: head [B,H,W,Cp] (requires_grad) is cut into the
    reference's NCHW outputs; the network's own Sigmoid cell (:168-169) is applied to hm -> (total, hm_loss, wh_loss, off_loss)"""
    nchw = head.permute(0, 3, 1, 2)
    logits = nchw[:, off_hm:off_hm + num_classes]
    output_hm = sigmoid_cell(logits)
    om = sigmoid_cell(-logits) if negated_sigmoid else None
    hm_loss = focal_loss(output_hm, example["hm"], om)
    wh_loss = reg_loss(nchw[:, off_wh:off_wh + 2], example["reg_mask"], example["ind"], example["wh"])
    off_loss = torch.zeros((), dtype=head.dtype)
    if off_reg != -1 and off_weight > 0:
        off_loss = reg_loss(nchw[:, off_reg:off_reg + 2], example["reg_mask"], example["ind"], example["reg"])
    return hm_weight * hm_loss + wh_weight * wh_loss + off_weight * off_loss, hm_loss, wh_loss, off_loss


def bf16_logits(rng, shp, limit, spread=3.0):
    """random logits inside +-limit, a share of them on the two limits, as the fp32 values of bf16 numbers"""
    x = np.clip(rng.normal(0, spread, shp), -limit, limit).astype(np.float32)
    far = rng.uniform(size=shp)
    x[far < 0.03] = -limit
    x[far > 0.97] = limit
    return torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()


def layout(C, reg_offset=True):
    """graphs.CenterNet.features: hm at 0, wh at C, reg at C + 2, Cp rounded up to 8"""
    return dict(num_classes=C, off_hm=0, off_wh=C, off_reg=C + 2 if reg_offset else -1), (C + 4 + 7) // 8 * 8


def hold_to_transcription(tag, head, tg, lay, weights, negated_sigmoid=False):
    want = cl.loss(head, tg["hm"], tg["ind"], tg["reg_mask"], tg["wh"], tg["reg"], **lay, **weights)
    h64 = torch.from_numpy(head).to(torch.float64).requires_grad_(True)
    ex = dict(hm=torch.from_numpy(tg["hm"]).double(), ind=torch.from_numpy(tg["ind"]).long(), reg_mask=torch.from_numpy(tg["reg_mask"]),
              wh=torch.from_numpy(tg["wh"]).double(), reg=torch.from_numpy(tg["reg"]).double())
    total, *parts = loss_cell(h64, ex, **lay, **weights, negated_sigmoid=negated_sigmoid)
    (g,) = torch.autograd.grad(total, h64)
    g = g.numpy()

    def rel(a, b):
        return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)

    assert rel(want["total"], total.detach()) <= 1e-12
    for got, ref in zip(want["parts"], parts):
        assert (got == 0 and float(ref.detach()) == 0) or rel(got, ref.detach()) <= 1e-12
    assert want["num_pos"][0] == float((tg["hm"] == 1).sum())
    assert np.array_equal(g == 0, want["grad"] == 0)                                          # structural zeros agree exactly
    nz = g != 0
    apart = cl.ulps_apart(g[nz].astype(np.float32), want["grad"][nz].astype(np.float32))
    print(f"cn_loss[{tag}]: total {float(want['total']):.6f}, non-zero gradients {int(nz.sum())}, differing after rounding to fp32 "
          f"{int((apart > 0).sum())}, worst {int(apart.max())} ulp")
    assert int(apart.max()) <= 1 and int((apart > 0).sum()) * 10000 <= int(nz.sum())
    return want


@pytest.mark.parametrize("name", ["small", "tiles", "plants"])
def test_contract_equals_the_reference_transcription_under_autograd(name):
    _, kw, tg = fixture_case(name)
    B, (W, H) = tg["hm"].shape[0], kw["feature_map_size"]
    lay, Cp = layout(kw["num_classes"])
    head = bf16_logits(np.random.default_rng(11), (B, H, W, Cp), 12.0)
    want = hold_to_transcription(name, head, tg, lay, WEIGHTS)
    assert want["num_pos"][0] > 0 and (want["parts"] > 0).all()


def test_contract_out_to_30_equals_the_transcription_with_the_negated_sigmoid():
    """beyond +-12 the literal 1 - sigmoid(x) has lost digits before the clip decides; out to +-30 the contract is held to the
    transcription with 1 - p written as the clipped sigmoid of the negated logit (as tests/test_pp_loss_cpu.py does for 1 - p_t)"""
    _, kw, tg = fixture_case("small")
    B, (W, H) = tg["hm"].shape[0], kw["feature_map_size"]
    lay, Cp = layout(kw["num_classes"])
    head = bf16_logits(np.random.default_rng(12), (B, H, W, Cp), 30.0, spread=8.0)
    hold_to_transcription("small, +-30", head, tg, lay, WEIGHTS, negated_sigmoid=True)
    assert (np.abs(head[..., :kw["num_classes"]]) >= 10).mean() > 0.2                         # many clipped cells


@pytest.mark.parametrize("variant", ["no offset head", "off_weight 0", "other weights", "no positives", "pred == target"])
def test_contract_variants_equal_the_transcription(variant):
    _, kw, tg = fixture_case("small")
    tg = {k: np.array(v) for k, v in tg.items()}
    B, (W, H) = tg["hm"].shape[0], kw["feature_map_size"]
    C = kw["num_classes"]
    lay, Cp = layout(C, reg_offset=variant != "no offset head")
    head = bf16_logits(np.random.default_rng(13), (B, H, W, Cp), 12.0)
    weights = dict(WEIGHTS)
    if variant == "off_weight 0":
        weights["off_weight"] = 0.0
    if variant == "other weights":
        weights = dict(hm_weight=float(np.float32(0.7)), wh_weight=float(np.float32(1.3)), off_weight=float(np.float32(2.5)))
    if variant == "no positives":
        tg["hm"] = np.where(tg["hm"] == 1, np.float32(0.5), tg["hm"])
    if variant == "pred == target":                                                           # bf16-representable targets, copied into the head
        for k in ("wh", "reg"):
            tg[k] = torch.from_numpy(tg[k]).to(torch.bfloat16).to(torch.float32).numpy()
        b, k = np.nonzero(tg["reg_mask"])
        i = tg["ind"][b, k]
        head.reshape(B, H * W, Cp)[b, i, C:C + 2] = tg["wh"][b, k]
        head.reshape(B, H * W, Cp)[b, i, C + 2:C + 4] = tg["reg"][b, k]
    want = hold_to_transcription(variant, head, tg, lay, weights)
    g = want["grad"]
    if variant in ("no offset head", "off_weight 0"):
        assert want["parts"][2] == 0 and not g[..., C + 2:].any() and g[..., C:C + 2].any()
    if variant == "no positives":
        assert want["num_pos"][0] == 0 and want["parts"][0] > 0
    if variant == "pred == target":
        shared = len(i) - len(np.unique(b * H * W + i))
        assert want["parts"][1] == 0 or shared > 0                                            # (slots sharing a cell keep one target each)
        assert np.count_nonzero(g[..., C:C + 4]) <= 8 * shared


def test_contract_skips_out_of_range_slots_as_if_masked():
    _, kw, tg = fixture_case("small")
    B, (W, H) = tg["hm"].shape[0], kw["feature_map_size"]
    lay, Cp = layout(kw["num_classes"])
    head = bf16_logits(np.random.default_rng(5), (B, H, W, Cp), 12.0)
    b, k = (int(v[0]) for v in np.nonzero(tg["reg_mask"]))
    masked = tg["reg_mask"].copy()
    masked[b, k] = 0
    want = cl.loss(head, tg["hm"], tg["ind"], masked, tg["wh"], tg["reg"], **lay, **WEIGHTS)
    for bad in (H * W, -1, -5, 2 ** 31 - 1):
        i2 = tg["ind"].copy()
        i2[b, k] = bad
        got = cl.loss(head, tg["hm"], i2, tg["reg_mask"], tg["wh"], tg["reg"], **lay, **WEIGHTS)
        for key in ("parts", "num_pos", "total", "grad"):
            assert np.array_equal(got[key], want[key]), (key, bad)
    loud = tg["reg_mask"] * 7                                                                 # a non-zero mask counts as 1
    got = cl.loss(head, tg["hm"], tg["ind"], loud.astype(np.uint8), tg["wh"], tg["reg"], **lay, **WEIGHTS)
    full = cl.loss(head, tg["hm"], tg["ind"], tg["reg_mask"], tg["wh"], tg["reg"], **lay, **WEIGHTS)
    assert np.array_equal(got["grad"], full["grad"]) and got["total"] == full["total"]
    odd = tg["hm"].copy()                                                                     # hm > 1 and NaN: in neither focal sum
    odd[0, 0, 0, 0], odd[0, 0, 0, 1] = 1.5, np.nan
    got = cl.loss(head, odd, tg["ind"], tg["reg_mask"], tg["wh"], tg["reg"], **lay, **WEIGHTS)
    assert np.isfinite(got["total"]) and got["grad"][0, 0, 0, 0] == 0 and got["grad"][0, 0, 1, 0] == 0 and not np.isnan(got["grad"]).any()


def test_loss_class_refuses_what_is_not_built():
    for bad in (dict(mse_loss=True), dict(dense_wh=True), dict(cat_spec_wh=True), dict(reg_loss="sl1"), dict(reg_loss="mse"), dict(num_stacks=2)):
        with pytest.raises(ValueError):
            det_ops.CenterNetLoss(80, **bad)
    ok = det_ops.CenterNetLoss(5, hm_weight=2.0, reg_offset=False)
    assert (ok.at.num_classes, ok.at.off_hm, ok.at.off_wh, ok.at.off_reg, ok.at.hm_weight) == (5, 0, 5, -1, 2.0)
    assert det_ops.cn_loss_workspace_bytes(16, 80, 128, 128) == 8 * 16 * (4 + 2 * 256) + 4 * 1280
    with pytest.raises(ValueError):
        det_ops.cn_loss(torch.zeros((1, 2, 2, 8)), {}, ok.at)                                 # the head has to be bf16


def test_loss_from_config_and_from_model_read_the_train_cfg():
    import os

    from minddet.models import Config, build_detector

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Config.fromfile(os.path.join(root, "configs", "centernet", "centernet_r18_dcn_train.py"))
    loss = det_ops.CenterNetLoss.from_config(cfg)
    assert (loss.num_classes, loss.hm_weight, loss.wh_weight, loss.off_weight, loss.reg_offset) == (80, 1.0, 0.1, 1.0, True)
    assert (loss.at.off_hm, loss.at.off_wh, loss.at.off_reg) == (0, 80, 82)
    assert det_ops.CenterNetLoss.from_config(cfg, num_classes=3).at.off_reg == 5
    net = build_detector(dict(cfg.model, num_classes=4), dict(cfg.train_cfg, loss=dict(cfg.train_cfg["loss"], off_weight=0.5)), cfg.test_cfg)
    at = net.loss_op().at
    assert (at.num_classes, at.off_wh, at.off_reg, at.off_weight) == (4, 4, 6, 0.5)
    with pytest.raises(ValueError):
        build_detector(cfg.model, dict(cfg.train_cfg, loss=dict(cfg.train_cfg["loss"], dense_wh=True)), cfg.test_cfg).loss_op()


def test_zero_hm_weight_gives_positive_zeros_in_the_contract():
    _, kw, tg = fixture_case("plants")
    lay, Cp = layout(kw["num_classes"])
    head = bf16_logits(np.random.default_rng(2), (1, 16, 16, Cp), 12.0)
    got = cl.loss(head, tg["hm"], tg["ind"], tg["reg_mask"], tg["wh"], tg["reg"], **lay, **dict(WEIGHTS, hm_weight=0.0))
    assert not got["grad"][..., :3].any() and not np.signbit(got["grad"][got["grad"] == 0]).any() and got["grad"][..., 3:7].any()
