"""CPU: the CenterPoint training loss without a GPU -- the ABI of include/minddet_hip_cploss.h (the two functions exported,
the semantic refusals answered before any device call, the ctypes mirrors laid out as the header says), the
contract tests/cp_loss_contract.py against a literal torch-float64 transcription of the reference's FastFocalLoss / RegLoss /
CenterHead.loss under autograd on the committed reference targets (tests/golden/cp_target_vectors.npz), and the config."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from minddet_amd import det_ops
from tests import cp_loss_contract as cl
from tests import abi_header as ah
from tests.abi_cases import B16, I, U8
from tests.abi_cases_cploss import CASES, CPLoss
from tests.abi_derive import attr, both, item, lib_handle, rc, refuse_single_defects, shape
from tests.test_cp_targets_cpu import fixture_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = ah.header("minddet_hip_cploss.h")
HDR_CP = ah.header("minddet_hip_cp.h")
WEIGHT = float(np.float32(0.25))
CODE_WEIGHTS = [float(np.float32(v)) for v in (1, 1, 1, 1, 1, 1, 0.2, 0.2, 1, 1)]     # the values an fp32 attribute struct carries


def test_header_declares_the_two_symbols_and_the_library_exports_them():
    assert ah.aot_symbols(HDR) == ["md_cp_loss", "md_cp_loss_grad"] and '#include "minddet_hip_cp.h"' in HDR
    assert "center_head.py:208-271" in HDR and "centernet_loss.py:22-82" in HDR
    assert "minddet_hip_cploss.h" in open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    assert {c.sym for c in CASES} == {"md_cp_loss", "md_cp_loss_grad"} and len({c.id for c in CASES}) == len(CASES)
    lib = lib_handle()
    for sym in ("md_cp_loss", "md_cp_loss_grad"):
        assert getattr(lib, sym)(0, None, None, None, None, None, None) == 1             # wrong parameter count, before anything else


def test_ctypes_mirrors_have_the_headers_layout():
    task = ah.struct_of("md_cp_task_attrs", HDR_CP)
    want = ah.struct_of("md_cp_loss_attrs", HDR, HDR_CP, known={"md_cp_task_attrs": task})
    assert C.sizeof(task) == 8 * 4 and C.sizeof(want) == 4 + 8 * 32 + 4 + 40

    for got in (det_ops._CPLossAttrs, CPLoss):
        assert ah.same_layout(got, want), got
    for got in (det_ops._CPTaskAttrs, dict(CPLoss._fields_)["task"]._type_):
        assert ah.layout(got) == ah.layout(task), got


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_cploss", case)


@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=[CASES[0].id, CASES[3].id])
def test_semantic_refusals_return_the_documented_codes(case):
    ARG, SIZE = 2, 4
    grad = case.sym == "md_cp_loss_grad"

    def task(t, name, value):
        return lambda c: setattr(c.extra.task[t], name, value)

    nan, inf = float("nan"), float("inf")
    edits = [
        attr("num_tasks", 0), attr("num_tasks", 9), attr("num_tasks", 1), attr("num_tasks", 3),
        task(1, "num_classes", 3), task(1, "num_classes", 1), task(0, "num_classes", 0),      # C != max(num_classes), no classes
        task(0, "off_reg", -1), task(1, "off_hm", 23), task(1, "off_dim", 22), task(0, "off_vel", -2), task(1, "off_rot", 24),
        task(1, "off_height", 24),                                                            # a head outside [0, Cp)
        task(1, "off_reg", 9), task(0, "off_hm", 9),                                          # two heads on one channel
        attr("weight", nan), attr("weight", inf), item("code_weights", 0, nan), item("code_weights", 9, -inf),
        shape(0, (0, 8, 12, 24), B16),                                                        # an empty batch
        shape(0, (2, 8, 12, 24), B16), shape(1, (1, 2, 2, 8, 11)), shape(1, (1, 2, 2, 9, 12)), shape(1, (1, 2, 1, 8, 12)),
        shape(1, (1, 3, 2, 8, 12)), shape(2, (1, 2, 4, 9)), shape(2, (1, 2, 5, 10)), shape(2, (2, 2, 4, 10)), shape(3, (1, 2, 5), I),
        shape(4, (1, 3, 4), U8), shape(5, (2, 2, 4), I), shape(6, (2, 11)), shape(6, (3, 12)), shape(7, (3,)), shape(8, (2,)),
    ]
    if grad:
        edits += [shape(9, (1, 8, 12, 16)), shape(9, (1, 12, 8, 24)), shape(9, (2, 8, 12, 24))]
    for i, e in enumerate(edits):
        assert rc(case, e) == ARG, i
    big = 1100                                                                                # M above the LDS bound
    grow = both(shape(2, (1, 2, big, 10)), shape(3, (1, 2, big), I), shape(4, (1, 2, big), U8), shape(5, (1, 2, big), I))
    assert rc(case, grow) == SIZE
    wide = both(shape(0, (1, 8, 12, 168), B16), *([shape(9, (1, 8, 12, 168))] if grad else []))   # Cp above the LDS bound
    assert rc(case, wide) == SIZE
    if "[workspace]" in case.id:
        assert rc(case, shape(len(case.operands) - 1, (223,), U8)) == SIZE                   # one byte short of 8 B T (12 + strips)


# ---------------------------------------------------------------------------------------------------- the reference, transcribed
def _transpose_and_gather_feat(feat, ind):
    feat = feat.permute(0, 2, 3, 1)
    feat = feat.reshape(feat.shape[0], -1, feat.shape[3])
    return feat.gather(1, ind.unsqueeze(2).expand(ind.shape[0], ind.shape[1], feat.shape[2]))


def reg_loss(output, mask, ind, target):
    """RegLoss.construct, centernet_loss.py:36-45"""
    pred = _transpose_and_gather_feat(output, ind)
    mask = mask.to(output.dtype).unsqueeze(2)
    loss = (pred * mask - target * mask).abs()
    loss = loss / (mask.sum() + 1e-4)
    return loss.permute(2, 1, 0).sum(2).sum(1)


def fast_focal_loss(out, target, ind, mask, cat):
    """FastFocalLoss.construct, centernet_loss.py:61-82"""
    mask = mask.to(out.dtype)
    gt = torch.pow(1 - target, 4)
    neg_loss = (torch.log(1 - out) * torch.pow(out, 2) * gt).sum()
    pos_pred_pix = _transpose_and_gather_feat(out, ind)
    pos_pred = pos_pred_pix.gather(2, cat.unsqueeze(2))
    num_pos = mask.sum()
    pos_loss = (torch.log(pos_pred) * torch.pow(1 - pos_pred, 2) * mask.unsqueeze(2)).sum()
    return -neg_loss if num_pos == 0 else -(pos_loss + neg_loss) / num_pos


def center_head_loss(head, example, task_offsets, num_classes, weight, code_weights):
    """CenterHead.loss, center_head.py:208-271, on float64: head [B,H,W,Cp] (requires_grad) is cut into the reference's per-task
    NCHW preds_dicts -> (total, per task (hm_loss, loc_loss, box_loss))"""
    widths = dict(reg=2, height=1, dim=3, rot=2, vel=2)
    total, rets = 0, []
    for t, (off, nc) in enumerate(zip(task_offsets, num_classes)):
        preds = {h: head[..., off[h]:off[h] + (nc if h == "hm" else widths[h])].permute(0, 3, 1, 2) for h in off}
        preds["hm"] = torch.clamp(torch.sigmoid(preds["hm"]), min=1e-4, max=1 - 1e-4)
        hm_loss = fast_focal_loss(preds["hm"], example["hm"][:, t, :nc], example["ind"][:, t], example["mask"][:, t], example["cat"][:, t])
        target_box = example["anno_box"][:, t]
        if "vel" in preds:
            anno = torch.cat((preds["reg"], preds["height"], preds["dim"], preds["vel"], preds["rot"]), 1)
            cw = code_weights
        else:
            anno = torch.cat((preds["reg"], preds["height"], preds["dim"], preds["rot"]), 1)
            target_box = target_box[..., [0, 1, 2, 3, 4, 5, -2, -1]]
            cw = code_weights[:8]
        box_loss = reg_loss(anno, example["mask"][:, t], example["ind"][:, t], target_box)
        loc_loss = (box_loss * torch.tensor(cw, dtype=head.dtype)).sum()
        total = total + hm_loss + weight * loc_loss
        rets.append((hm_loss, loc_loss, box_loss))
    return total, rets


def head_layout(num_classes, vel=True):
    """heads side by side in the order of graphs.SEPHEAD_ORDER -> (per task {head: first channel}, Cp rounded up to 8)"""
    offs, base = [], 0
    for nc in num_classes:
        off = {}
        for h, w in (("reg", 2), ("height", 1), ("dim", 3), ("rot", 2), ("vel", 2), ("hm", nc)):
            if h == "vel" and not vel:
                continue
            off[h] = base
            base += w
        offs.append(off)
    return offs, (base + 7) // 8 * 8


def bf16_logits(rng, shape, spread=3.0):
    """random logits, a share of them far out on both sides, as the fp32 values of bf16 numbers"""
    x = rng.normal(0, spread, shape).astype(np.float32)
    far = rng.uniform(size=shape)
    x[far < 0.03] = -30.0
    x[far > 0.97] = 30.0
    return torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()


@pytest.mark.parametrize("name,vel", [("small", True), ("plants", True), ("small", False)])
def test_contract_equals_the_reference_transcription_under_autograd(name, vel):
    _, _, ncs, kw, tg = fixture_case(name)
    B, (W, H) = tg["hm"].shape[0], kw["feature_map_size"]
    offs, Cp = head_layout(ncs, vel)
    head = bf16_logits(np.random.default_rng(11), (B, H, W, Cp))
    cws = CODE_WEIGHTS if vel else CODE_WEIGHTS[:8]
    want = cl.loss(head, tg["hm"], tg["anno_box"], tg["ind"], tg["mask"], tg["cat"], task_offsets=offs, num_classes=ncs, weight=WEIGHT,
                   code_weights=cws)
    h64 = torch.from_numpy(head).to(torch.float64).requires_grad_(True)
    ex = dict(hm=torch.from_numpy(tg["hm"]).double(), anno_box=torch.from_numpy(tg["anno_box"]).double(),
              ind=torch.from_numpy(tg["ind"]).long(), mask=torch.from_numpy(tg["mask"]), cat=torch.from_numpy(tg["cat"]).long())
    total, rets = center_head_loss(h64, ex, offs, ncs, WEIGHT, cws)
    (g,) = torch.autograd.grad(total, h64)
    g = g.numpy()

    def rel(a, b):
        return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)

    assert rel(want["total"], total.detach()) <= 1e-12
    for t, (hm_loss, loc_loss, box_loss) in enumerate(rets):
        assert rel(want["parts"][t, 0], hm_loss.detach()) <= 1e-12 and rel(want["parts"][t, 1], loc_loss.detach()) <= 1e-12
        box = box_loss.detach().numpy()
        assert np.allclose(want["parts"][t, 2:2 + len(box)], box, rtol=1e-12, atol=0) and not want["parts"][t, 2 + len(box):].any()
        assert want["num_pos"][t] == float(tg["mask"][:, t].sum())
    assert np.array_equal(g == 0, want["grad"] == 0)                                          # zeros agree exactly
    nz = g != 0
    apart = cl.ulps_apart(g[nz].astype(np.float32), want["grad"][nz].astype(np.float32))
    print(f"cp_loss[{name}, vel={vel}]: non-zero gradients {int(nz.sum())}, differing after rounding to fp32 {int((apart > 0).sum())}, "
          f"worst {int(apart.max())} ulp; clipped hm cells {int((np.abs(head) >= 10).sum())}")
    assert int(apart.max()) <= 1 and int((apart > 0).sum()) * 10000 <= int(nz.sum())
    assert int(nz.sum()) > 500 and want["num_pos"].sum() > 0


def test_contract_skips_out_of_range_slots_as_if_masked():
    _, _, ncs, kw, tg = fixture_case("small")
    B, (W, H) = tg["hm"].shape[0], kw["feature_map_size"]
    offs, Cp = head_layout(ncs)
    head = bf16_logits(np.random.default_rng(5), (B, H, W, Cp))
    args = dict(task_offsets=offs, num_classes=ncs, weight=WEIGHT, code_weights=CODE_WEIGHTS)
    ind, mask, cat = tg["ind"].copy(), tg["mask"].copy(), tg["cat"].copy()
    b, t, k = (int(v[0]) for v in np.nonzero(mask))
    masked = mask.copy()
    masked[b, t, k] = 0
    want = cl.loss(head, tg["hm"], tg["anno_box"], ind, masked, cat, **args)
    for bad_ind, bad_cat in ((H * W, cat[b, t, k]), (-1, cat[b, t, k]), (ind[b, t, k], ncs[t]), (ind[b, t, k], -1)):
        i2, c2 = ind.copy(), cat.copy()
        i2[b, t, k], c2[b, t, k] = bad_ind, bad_cat
        got = cl.loss(head, tg["hm"], tg["anno_box"], i2, mask, c2, **args)
        for key in ("parts", "num_pos", "total", "grad"):
            assert np.array_equal(got[key], want[key]), (key, bad_ind, bad_cat)


def test_train_config_builds_the_loss():
    from minddet.models import Config
    from minddet_amd import graphs

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc_train.py"))
    assert cfg.train_cfg["loss"] == dict(weight=0.25, code_weights=[1, 1, 1, 1, 1, 1, 0.2, 0.2, 1, 1])
    head = graphs.CenterHead(**{k: v for k, v in cfg.model["bbox_head"].items() if k != "type"})
    assert head.weight == 0.25 and head.code_weights == [1.0] * 10
    loss = det_ops.CenterPointLoss.from_config(cfg, head)
    at = loss.at
    assert at.num_tasks == 6 and abs(at.weight - 0.25) < 1e-7 and [round(float(v), 4) for v in at.code_weights] == [1, 1, 1, 1, 1, 1, 0.2, 0.2, 1, 1]
    offs = head.task_offsets()
    for t in range(6):
        a = at.task[t]
        assert (a.off_reg, a.off_height, a.off_dim, a.off_rot, a.off_vel, a.off_hm) == tuple(offs[t][h] for h in ("reg", "height", "dim", "rot", "vel", "hm"))
        assert a.num_classes == head.num_classes[t]
    kept = graphs.CenterHead(**{k: v for k, v in cfg.model["bbox_head"].items() if k != "type"}, weight=0.5, code_weights=[2.0] * 10)
    assert det_ops.CenterPointLoss.from_head(kept).weight == 0.5 and det_ops.CenterPointLoss.from_head(kept).code_weights == [2.0] * 10
    assert det_ops.cp_loss_workspace_bytes(4, 6, 128, 128) == 8 * 4 * 6 * (12 + 256)
    with pytest.raises(ValueError):
        det_ops.cp_loss_attrs(offs, head.num_classes, 0.25, [1.0] * 8)                       # heads with vel need ten code weights
