"""-m gpu: md_cn_loss / md_cn_loss_grad (det_ops.cn_loss, csrc/cnloss.hip) against tests/cn_loss_contract.py, which the CPU tests show
equal to a literal transcription of the reference's loss under autograd.

Conditions: the three parts, num_pos and total within 1 fp32 ulp of the contract's float64 value rounded to fp32; grad exactly 0
wherever the contract's is and NaN nowhere; elsewhere within 1 ulp of the rounded contract value, with at most 1 in 10^4 of the non-zero
elements differing at all (the cap and its reason are those of tests/test_cp_loss_gpu.py); md_cn_loss bit-identical to md_cn_loss_grad
in parts / num_pos / total.  Then: the layout without an offset head, a batch without objects, the fixture's own targets, the channel
order pinned by perturbing one head channel at a time, equal results across calls, streams and the scratch-pool form with
garbage-filled outputs, autograd through det_ops.center_net_loss, and the production shape."""
import functools

import numpy as np
import pytest
import torch

from tests import cn_loss_contract as cl
from tests.conftest import has_gpu
from tests.test_cn_loss_cpu import WEIGHTS, bf16_logits, layout
from tests.test_cn_targets_cpu import fixture_case

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
KEYS = ("hm", "ind", "reg_mask", "wh", "reg")


class Problem:
    """one call's inputs as numpy (head: the fp32 values of the bf16 logits; the padding channels get a bf16 NaN on the device) and the
    contract's result, computed once and shared read-only"""

    def __init__(self, head, targets, lay, weights=WEIGHTS):
        self.head, self.targets, self.lay, self.weights = head, targets, dict(lay), dict(weights)
        C = lay["num_classes"]
        used = set(range(lay["off_hm"], lay["off_hm"] + C)) | {lay["off_wh"], lay["off_wh"] + 1}
        if lay["off_reg"] != -1:
            used |= {lay["off_reg"], lay["off_reg"] + 1}
        self.pad = np.setdiff1d(np.arange(head.shape[3]), sorted(used))
        self.want = cl.loss(head, *(targets[k] for k in KEYS), **self.lay, **self.weights)
        for v in list(self.want.values()) + [head] + list(targets.values()):
            v.setflags(write=False)

    def device(self, head=None):
        from minddet_amd import det_ops

        h = torch.from_numpy(np.array(self.head if head is None else head))
        h[..., torch.from_numpy(self.pad)] = float("nan")                     # the pad channels never enter the arithmetic
        tg = {k: torch.from_numpy(np.array(self.targets[k])).to(DEV) for k in KEYS}
        lay = self.lay
        at = det_ops.cn_loss_attrs(lay["num_classes"], lay["off_hm"], lay["off_wh"], None if lay["off_reg"] == -1 else lay["off_reg"],
                                   reg_offset=lay["off_reg"] != -1, **self.weights)
        return h.to(torch.bfloat16).to(DEV), tg, at


def to_np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check(tag, got, want):
    """the conditions of the module docstring; prints the measured figures before it asserts"""
    worst = cl.compare_losses(got, want)
    nnz, ndiff, worst_g, wrong_zero, nans = cl.compare_grad(got["grad"], want["grad"])
    print(f"cn_loss[{tag}]: total {float(got['total'][0]):.6f}, num_pos {float(got['num_pos'][0]):.0f}, losses worst {worst} ulp; grad "
          f"non-zero {nnz}, differing {ndiff}, worst {worst_g} ulp, non-zero where the contract is zero {wrong_zero}, NaN {nans}")
    assert worst <= 1
    assert wrong_zero == 0 and nans == 0
    assert worst_g <= 1 and ndiff * 10000 <= nnz, (worst_g, ndiff, nnz)


def run(pr, grad=True, out=None, head=None):
    from minddet_amd import det_ops

    h, tg, at = pr.device(head)
    return det_ops.cn_loss(h, tg, at, grad=grad, out=out)


def planted_targets(rng, B, C, H, W, M):
    HW = H * W
    hm = (rng.uniform(size=(B, C, H, W)) ** 4).astype(np.float32)
    ind = rng.integers(0, HW, (B, M)).astype(np.int32)
    mask = (rng.uniform(size=(B, M)) < 0.7).astype(np.uint8)
    mask[:, :6] = 1
    wh = rng.uniform(0.5, 20, (B, M, 2)).astype(np.float32)
    reg = rng.uniform(0, 1, (B, M, 2)).astype(np.float32)
    return hm, ind, mask, wh, reg


@functools.lru_cache(maxsize=None)
def main_problem():
    """B = 2, C = 3 (Cp = 8: one padding channel), 9 x 37 cells (an odd row pitch, 333 = 5 strips + 13), M = 16, with everything the
    issue plants"""
    rng = np.random.default_rng(2025)
    B, C, H, W, M = 2, 3, 9, 37, 16
    HW = H * W
    lay, Cp = layout(C)
    assert Cp == 8
    head = bf16_logits(rng, (B, H, W, Cp), 30.0, spread=4.0)                  # logits out to +-30: clipped cells on both sides
    hm, ind, mask, wh, reg = planted_targets(rng, B, C, H, W, M)
    ind[0, 1] = ind[0, 0]                                                     # two slots on one cell
    for b, k in ((0, 0), (0, 2), (1, 0), (1, 3), (1, 4)):                     # centre cells as the assigner leaves them
        hm[b, k % C, ind[b, k] // W, ind[b, k] % W] = 1.0
    head[0, 0, 0, 0], head[0, 0, 1, 1], head[0, 0, 2, 2] = 0.0, 30.0, -30.0   # logits 0 and +-30 ...
    hm[0, 0, 0, 0], hm[0, 1, 0, 1], hm[0, 2, 0, 2] = 0.25, 1.0, 1.0           # ... on a negative and on two positives
    head[1, 0, 3, 0], head[1, 0, 4, 0], hm[1, 0, 0, 3], hm[1, 0, 0, 4] = 30.0, -30.0, 0.5, 0.5
    hm[1, 1, 2, 5], hm[1, 1, 2, 6], hm[1, 1, 2, 7] = 1.5, np.nan, np.float32(1) - np.float32(2) ** -24   # > 1, NaN, just below 1
    head[1, 2, 5:8, 1] = 0.5
    mask[0, 5], ind[0, 5] = 0, -5                                             # a masked slot with a bad ind
    mask[0, 7], ind[0, 7], mask[1, 7], ind[1, 7] = 1, HW, 1, np.iinfo(np.int32).max   # set masks on out-of-range cells
    mask[1, 8], ind[1, 8], mask[1, 9] = 1, -1, 3                              # ... and a mask value other than 1 on a valid slot
    b, k = 1, 2                                                               # pred == target (bf16-representable) on one valid slot
    mask[b, k] = 1
    wh[b, k], reg[b, k] = (3.5, 12.0), (0.25, 0.5)
    head[b, ind[b, k] // W, ind[b, k] % W, C:C + 4] = (3.5, 12.0, 0.25, 0.5)
    pr = Problem(head, dict(hm=hm, ind=ind, reg_mask=mask, wh=wh, reg=reg), lay)
    assert pr.want["num_pos"][0] >= 7 and len(pr.pad) == 1 and (np.abs(head[..., :C]) >= 30).sum() > 50
    return pr


def test_main_shape_equals_the_contract_and_forward_only_equals_forward_with_grad():
    pr = main_problem()
    got = to_np(run(pr))
    check("main", got, pr.want)
    fwd = to_np(run(pr, grad=False))
    assert set(fwd) == {"total", "parts", "num_pos"}
    for k in fwd:
        assert np.array_equal(bits(fwd[k]), bits(got[k])), k
    g = got["grad"]
    assert g[0, 0, 1, 1] == 0 and g[0, 0, 2, 2] == 0 and g[0, 0, 0, 0] != 0 and g[1, 0, 3, 0] == 0 and g[1, 0, 4, 0] == 0   # the clip
    assert g[1, 2, 5, 1] == 0 and g[1, 2, 6, 1] == 0 and g[1, 2, 7, 1] != 0                 # hm > 1, NaN: in neither sum
    assert not np.signbit(g[g == 0]).any() and not g[..., 7].any()                          # +0.0, the padding channel included


def test_layout_without_an_offset_head():
    """C = 5 (Cp = 16: seven padding channels), off_reg = -1"""
    rng = np.random.default_rng(7)
    B, C, H, W, M = 1, 5, 6, 11, 8
    lay, Cp = layout(C, reg_offset=False)
    head = bf16_logits(rng, (B, H, W, 16), 30.0)
    hm, ind, mask, wh, reg = planted_targets(rng, B, C, H, W, M)
    hm[0, 1, 2, 3] = hm[0, 4, 5, 10] = 1.0
    pr = Problem(head, dict(hm=hm, ind=ind, reg_mask=mask, wh=wh, reg=reg), lay)
    assert len(pr.pad) == 9 and Cp == 16
    got = to_np(run(pr))
    check("no offset head", got, pr.want)
    assert got["parts"][2] == 0 and not got["grad"][..., 7:].any() and got["grad"][..., 5:7].any()
    zero_w = Problem(head, pr.targets, layout(C)[0], dict(WEIGHTS, off_weight=0.0))         # an offset head, off_weight 0
    got0 = to_np(run(zero_w))
    check("off_weight 0", got0, zero_w.want)
    assert got0["parts"][2] == 0 and not got0["grad"][..., 7:].any()


def test_batch_without_objects():
    rng = np.random.default_rng(8)
    B, C, H, W, M = 2, 3, 5, 13, 4
    lay, Cp = layout(C)
    head = bf16_logits(rng, (B, H, W, Cp), 12.0)
    hm = np.zeros((B, C, H, W), np.float32)
    z = dict(hm=hm, ind=np.zeros((B, M), np.int32), reg_mask=np.zeros((B, M), np.uint8), wh=np.zeros((B, M, 2), np.float32),
             reg=np.zeros((B, M, 2), np.float32))
    pr = Problem(head, z, lay)
    got = to_np(run(pr))
    check("no objects", got, pr.want)
    assert got["num_pos"][0] == 0 and got["parts"][0] > 0 and got["parts"][1] == 0 and got["parts"][2] == 0
    assert not got["grad"][..., C:].any()


def test_fixture_targets_equal_the_contract():
    _, kw, tg = fixture_case("small")
    B, (W, H) = tg["hm"].shape[0], kw["feature_map_size"]
    lay, Cp = layout(kw["num_classes"])
    head = bf16_logits(np.random.default_rng(40), (B, H, W, Cp), 30.0)
    pr = Problem(head, {k: np.array(tg[k]) for k in KEYS}, lay)
    check("small fixture", to_np(run(pr)), pr.want)


def test_channel_order_follows_the_offsets():
    """regression channels at the slots' cells equal to the (bf16-representable) targets: wh_loss == off_loss == 0 and no regression
    gradient; one head channel moved by 0.5 at one slot's cell moves exactly the matching loss and gradient element"""
    rng = np.random.default_rng(3)
    B, C, H, W, M = 1, 3, 4, 5, 4
    lay, Cp = layout(C)
    head = bf16_logits(rng, (B, H, W, Cp), 12.0, spread=1.0)
    wh = torch.from_numpy(rng.uniform(1, 9, (B, M, 2)).astype(np.float32)).to(torch.bfloat16).to(torch.float32).numpy()
    reg = torch.from_numpy(rng.uniform(0, 1, (B, M, 2)).astype(np.float32)).to(torch.bfloat16).to(torch.float32).numpy()
    ind = np.array([[3, 11, 18, 0]], np.int32)
    mask = np.array([[1, 1, 1, 0]], np.uint8)
    hm = (rng.uniform(size=(B, C, H, W)) ** 4).astype(np.float32)
    for k in range(3):
        head[0, ind[0, k] // W, ind[0, k] % W, C:C + 2] = wh[0, k]
        head[0, ind[0, k] // W, ind[0, k] % W, C + 2:C + 4] = reg[0, k]
    pr = Problem(np.array(head), dict(hm=hm, ind=ind, reg_mask=mask, wh=wh, reg=reg), lay)
    got = to_np(run(pr))
    assert got["parts"][1] == 0 and got["parts"][2] == 0 and not got["grad"][..., C:].any()
    y, x = 11 // W, 11 % W
    den = 2 * 3 + 1e-4
    for ch, part, weight in ((C, 1, WEIGHTS["wh_weight"]), (C + 1, 1, WEIGHTS["wh_weight"]), (C + 2, 2, 1.0), (C + 3, 2, 1.0)):
        moved = np.array(head)
        moved[0, y, x, ch] = float(torch.tensor(float(moved[0, y, x, ch]) + 0.5).to(torch.bfloat16))
        delta = abs(float(moved[0, y, x, ch]) - float(head[0, y, x, ch]))
        g = to_np(run(pr, head=moved))
        other = 3 - part
        assert delta > 0.25 and g["parts"][other] == 0 and abs(g["parts"][part] - delta / den) <= 2e-7 * g["parts"][part], (ch, g["parts"])
        gr = g["grad"][0]
        assert np.argwhere(gr[..., C:] != 0).tolist() == [[y, x, ch - C]]
        assert abs(gr[y, x, ch] - weight / den) <= 2e-7 * weight


def test_equal_across_calls_streams_and_the_scratch_pool_with_garbage_filled_outputs():
    from minddet_amd import _lib, det_ops

    pr = main_problem()
    h, tg, at = pr.device()
    first = to_np(run(pr))

    def garbage():
        out = dict(total=torch.empty((1,), device=DEV), parts=torch.empty((3,), device=DEV), num_pos=torch.empty((1,), device=DEV),
                   grad=torch.empty(tuple(h.shape), device=DEV))
        for v in out.values():
            v.view(torch.uint8).fill_(0xFF)
        return out

    again = to_np(run(pr, out=garbage()))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs, pool, fwd = [garbage(), garbage()], [garbage(), garbage()], [garbage(), garbage()]
    torch.cuda.synchronize()
    for rep in range(2):                                                      # the second round reuses each stream's pool buffer
        for s, o, q, f in zip(streams, outs, pool, fwd):
            with torch.cuda.stream(s):
                det_ops.cn_loss(h, tg, at, grad=True, out=o)
                ops = [h] + [tg[k] for k in KEYS]
                assert _lib.call("md_cn_loss_grad", ops + [q["parts"], q["num_pos"], q["total"], q["grad"]], extra=at) == 0
                assert _lib.call("md_cn_loss", ops + [f["parts"], f["num_pos"], f["total"]], extra=at) == 0
    for o in [again] + [to_np(o) for o in outs + pool]:
        for k in ("total", "parts", "num_pos", "grad"):
            assert np.array_equal(bits(first[k]), bits(o[k])), k               # (a surviving 0xFF byte would differ from `first`)
    for f in fwd:
        f = to_np(f)
        for k in ("total", "parts", "num_pos"):
            assert np.array_equal(bits(first[k]), bits(f[k])), k
    check("main, again", first, pr.want)


def test_autograd_through_center_net_loss():
    from minddet_amd import det_ops

    pr = main_problem()
    h, tg, at = pr.device()
    loss = det_ops.CenterNetLoss(3, **WEIGHTS)
    ref = run(pr)
    x = h.clone().requires_grad_(True)
    total, parts, num_pos = det_ops.center_net_loss(x, tg, loss)
    assert total.requires_grad and not parts.requires_grad and not num_pos.requires_grad
    up = torch.tensor([2.5], device=DEV)
    (g,) = torch.autograd.grad(total, x, grad_outputs=up)
    torch.cuda.synchronize()
    assert g.dtype == torch.bfloat16 and g.shape == x.shape
    assert torch.equal(total.detach(), ref["total"]) and torch.equal(parts, ref["parts"]) and torch.equal(num_pos, ref["num_pos"])
    want = (ref["grad"] * 2.5).to(torch.bfloat16)
    assert torch.equal(g.view(torch.int16), want.view(torch.int16)) and bool((g != 0).any())
    y = h.clone().requires_grad_(True)
    (det_ops.center_net_loss(y, tg, loss)[0].sum() * 0.5).backward()
    assert torch.equal(y.grad.view(torch.int16), (ref["grad"] * 0.5).to(torch.bfloat16).view(torch.int16))


def test_production_shape_equals_the_contract():
    """B = 16, 80 classes on 128 x 128 (Cp = 88), max_objs 128: targets from det_ops.cn_assign_targets on about ten seeded objects per
    image, seeded bf16 logits around the head's initial bias"""
    from minddet_amd import det_ops

    rng = np.random.default_rng(1600)
    B, G, C, HW = 16, 128, 80, 128
    c = rng.uniform(0, 128, (B, G, 2))
    s = np.exp(rng.uniform(np.log(2.0), np.log(90.0), (B, G, 2)))
    boxes = np.concatenate([c - s / 2, c + s / 2], -1).astype(np.float32)
    classes = np.where(rng.uniform(size=(B, G)) < 10 / G, rng.integers(1, C + 1, (B, G)), 0).astype(np.int32)
    targets = det_ops.cn_assign_targets(torch.from_numpy(boxes).to(DEV), torch.from_numpy(classes).to(DEV), num_classes=C,
                                        feature_map_size=(HW, HW), max_objs=G)
    head = torch.from_numpy(rng.normal(-2.19, 2.0, (B, HW, HW, 88)).astype(np.float32)).to(torch.bfloat16).to(DEV)
    loss = det_ops.CenterNetLoss(C, **WEIGHTS)
    got = to_np(loss(head, targets, grad=True))
    fwd = to_np(loss(head, targets))
    tg = {k: targets[k].cpu().numpy() for k in KEYS}
    want = cl.loss(head.to(torch.float32).cpu().numpy(), *(tg[k] for k in KEYS), **layout(C)[0], **WEIGHTS)
    assert 100 < want["num_pos"][0] < 300 and head.shape == (16, 128, 128, 88)
    check("coco b16", got, want)
    for k in fwd:
        assert np.array_equal(bits(fwd[k]), bits(got[k])), k


def scattered_problem(Cp, lay, seed, shape=(2, 5, 13), M=6, weights=WEIGHTS):
    """a small problem on a head of Cp channels whose heads sit where `lay` says, everything else NaN padding"""
    rng = np.random.default_rng(seed)
    B, H, W = shape
    C = lay["num_classes"]
    head = bf16_logits(rng, (B, H, W, Cp), 30.0)
    hm, ind, mask, wh, reg = planted_targets(rng, B, C, H, W, M)
    hm[0, 0, 1, 2] = hm[1, C - 1, 4, 12] = 1.0
    ind[1, 1] = ind[1, 0]
    return Problem(head, dict(hm=hm, ind=ind, reg_mask=mask, wh=wh, reg=reg), lay, weights)


@pytest.mark.parametrize("Cp", [7, 9])
def test_channel_counts_that_are_no_multiple_of_eight(Cp):
    """the element-wise staging of the head strip and of the grad strip: Cp = 7 (no padding channel) and Cp = 9"""
    pr = scattered_problem(Cp, dict(num_classes=3, off_hm=2, off_wh=0, off_reg=5), 70 + Cp)
    assert len(pr.pad) == Cp - 7
    got = to_np(run(pr))
    check(f"Cp = {Cp}", got, pr.want)
    fwd = to_np(run(pr, grad=False))
    for k in fwd:
        assert np.array_equal(bits(fwd[k]), bits(got[k])), k


def test_widest_head_and_heads_in_another_order():
    """Cp = 160, the bound of the LDS staging (61.5 KB of dynamic LDS with the gradient), the heads far apart and reg in front of hm"""
    pr = scattered_problem(160, dict(num_classes=3, off_hm=150, off_wh=10, off_reg=77), 160)
    assert len(pr.pad) == 153
    got = to_np(run(pr))
    check("Cp = 160", got, pr.want)
    assert got["grad"][..., 150:153].any() and got["grad"][..., 10:12].any() and got["grad"][..., 77:79].any()


def test_operands_that_are_not_16_byte_aligned():
    """head and grad two / four bytes past a 16-byte boundary, hm four bytes past one: the scalar forms of the staging and of the count"""
    from minddet_amd import _lib

    pr = main_problem()
    h, tg, at = pr.device()
    want = run(pr)

    def shifted(t):
        buf = torch.empty((t.numel() + 1,), dtype=t.dtype, device=DEV)
        view = buf[1:].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        return view

    h2, hm2 = shifted(h), shifted(tg["hm"])
    out = dict(parts=torch.empty((3,), device=DEV), num_pos=torch.empty((1,), device=DEV), total=torch.empty((1,), device=DEV),
               grad=shifted(torch.empty(tuple(h.shape), device=DEV)))
    ops = [h2, hm2] + [tg[k] for k in KEYS[1:]]
    assert _lib.call("md_cn_loss_grad", ops + [out["parts"], out["num_pos"], out["total"], out["grad"]], extra=at) == 0
    got, want = to_np(out), to_np(want)
    for k in ("total", "parts", "num_pos", "grad"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    check("unaligned", got, pr.want)


def test_zero_hm_weight_leaves_positive_zeros():
    pr = scattered_problem(8, layout(3)[0], 9, weights=dict(WEIGHTS, hm_weight=0.0))
    got = to_np(run(pr))
    check("hm_weight 0", got, pr.want)
    assert not got["grad"][..., :3].any() and not np.signbit(got["grad"][got["grad"] == 0]).any() and got["grad"][..., 3:7].any()


def test_model_loss_runs_features_then_the_loss():
    """graphs.CenterNet.loss(images, example, grad): features() and then cn_loss with the loss of the config's train_cfg"""
    import os

    from minddet.models import Config
    from minddet_amd import det_ops, graphs

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Config.fromfile(os.path.join(root, "configs", "centernet", "centernet_r18_dcn_train.py"))
    train_cfg = dict(cfg.train_cfg, loss=dict(cfg.train_cfg["loss"], wh_weight=0.25))
    net = graphs.CenterNet(depth=18, num_classes=5, dcn=False, train_cfg=train_cfg).to(DEV)
    g = torch.Generator().manual_seed(4)
    x = torch.zeros((2, 64, 96, 8))
    x[..., :3] = torch.randn((2, 64, 96, 3), generator=g)
    images = x.to(torch.bfloat16).to(DEV)
    rng = np.random.default_rng(4)
    c = rng.uniform(2, 14, (2, 6, 2)) * (1.5, 1.0)
    s = rng.uniform(2, 9, (2, 6, 2))
    boxes = np.concatenate([c - s / 2, c + s / 2], -1).astype(np.float32)
    example = det_ops.cn_assign_targets(torch.from_numpy(boxes).to(DEV), torch.from_numpy(rng.integers(1, 6, (2, 6)).astype(np.int32)).to(DEV),
                                        num_classes=5, feature_map_size=(24, 16), max_objs=8)
    out = net.loss(images, example, grad=True)
    head = net.features(images)
    assert set(out) == {"total", "parts", "num_pos", "grad", "head"} and out["head"].shape == (2, 16, 24, 16) and torch.equal(out["head"], head)
    loss = net.loss_op()
    assert abs(loss.at.wh_weight - 0.25) < 1e-7 and (loss.at.num_classes, loss.at.off_wh, loss.at.off_reg) == (5, 5, 7)
    direct = det_ops.cn_loss(head, example, loss.at, grad=True)
    for k in ("total", "parts", "num_pos", "grad"):
        assert torch.equal(out[k], direct[k]), k
    fwd = net.loss(images, example)
    assert "grad" not in fwd and torch.equal(fwd["total"], out["total"])
    tg = {k: example[k].cpu().numpy() for k in KEYS}
    want = cl.loss(head.to(torch.float32).cpu().numpy(), *(tg[k] for k in KEYS), **layout(5)[0], **dict(WEIGHTS, wh_weight=0.25))
    check("model", to_np({k: out[k] for k in ("total", "parts", "num_pos", "grad")}), want)
    assert float(out["num_pos"][0]) >= 6
