"""-m gpu: md_cp_loss / md_cp_loss_grad (det_ops.cp_loss, csrc/cploss.hip) against tests/cp_loss_contract.py, which the CPU tests show
equal to a literal transcription of the reference's loss under autograd.

Conditions: parts, num_pos and total within 1 fp32 ulp of the contract's float64 value rounded to fp32; grad exactly 0 wherever the
contract's is and NaN nowhere; elsewhere within 1 ulp of the rounded contract value, with at most 1 in 10^4 of the non-zero elements
differing at all (the cap and its reason are those of tests/test_cp_targets_gpu.py: two float64 evaluations that are each good to an
ulp of float64 round to different fp32 neighbours on about 2^-27 of the values; an fp32 evaluation would differ on a large share);
md_cp_loss bit-identical to md_cp_loss_grad in parts / num_pos / total.  Then: the shape without vel, the column order pinned by
perturbing one head channel at a time, equal results across calls, streams and the scratch-pool form with garbage-filled outputs,
autograd through det_ops.center_point_loss, and the production shape."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import cp_loss_contract as cl
from tests.conftest import has_gpu
from tests.test_cp_loss_cpu import CODE_WEIGHTS, WEIGHT, bf16_logits, head_layout
from tests.test_cp_targets_cpu import fixture_case

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("hm", "anno_box", "ind", "mask", "cat")


class Problem:
    """one call's inputs as numpy (head: the fp32 values of the bf16 logits; pad: which channels get a bf16 NaN on the device) and the
    contract's result, computed once and shared read-only"""

    def __init__(self, head, targets, offs, ncs, code_weights, weight=WEIGHT):
        self.head, self.targets, self.offs, self.ncs, self.cw, self.weight = head, targets, offs, ncs, list(code_weights), weight
        used = sorted({c for off, nc in zip(offs, ncs) for h, c0 in off.items() for c in range(c0, c0 + dict(reg=2, height=1, dim=3, rot=2,
                                                                                                           vel=2, hm=nc)[h])})
        self.pad = np.setdiff1d(np.arange(head.shape[3]), used)
        self.want = cl.loss(head, *(targets[k] for k in KEYS), task_offsets=offs, num_classes=ncs, weight=weight, code_weights=self.cw)
        for v in list(self.want.values()) + [head] + list(targets.values()):
            v.setflags(write=False)

    def device(self, head=None):
        from minddet_amd import det_ops

        h = torch.from_numpy(np.array(self.head if head is None else head))
        h[..., torch.from_numpy(self.pad)] = float("nan")                     # the pad channels never enter the arithmetic
        tg = {k: torch.from_numpy(np.array(self.targets[k])).to(DEV) for k in KEYS}
        return h.to(torch.bfloat16).to(DEV), tg, det_ops.cp_loss_attrs(self.offs, self.ncs, self.weight, self.cw)


def to_np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check(tag, got, want):
    """the conditions of the module docstring; prints the measured figures before it asserts"""
    worst = cl.compare_losses(got, want)
    nnz, ndiff, worst_g, wrong_zero, nans = cl.compare_grad(got["grad"], want["grad"])
    print(f"cp_loss[{tag}]: total {float(got['total'][0]):.6f}, losses worst {worst} ulp; grad non-zero {nnz}, differing {ndiff}, worst "
          f"{worst_g} ulp, non-zero where the contract is zero {wrong_zero}, NaN {nans}")
    assert worst <= 1
    assert wrong_zero == 0 and nans == 0
    assert worst_g <= 1 and ndiff * 10000 <= nnz, (worst_g, ndiff, nnz)


@functools.lru_cache(maxsize=None)
def main_problem():
    """B = 2, tasks of (1, 2, 2) classes with vel (35 channels, Cp = 40), 9 x 37 cells (an odd row pitch, 333 = 5 strips + 13), M = 16,
    with everything the issue plants"""
    rng = np.random.default_rng(2024)
    B, H, W, M, ncs = 2, 9, 37, 16, [1, 2, 2]
    HW, T, C = H * W, 3, 2
    offs, Cp = head_layout(ncs)
    assert Cp == 40
    head = bf16_logits(rng, (B, H, W, Cp))                                    # logits out to +-30: clipped cells on both sides
    hm = (rng.uniform(size=(B, T, C, H, W)) ** 4).astype(np.float32)
    hm[:, 0, 1] = np.nan                                                      # the plane the one-class task does not have
    anno = rng.normal(0, 1.5, (B, T, M, 10)).astype(np.float32)
    ind = rng.integers(0, HW, (B, T, M)).astype(np.int32)
    cat = np.stack([rng.integers(0, nc, (B, M)) for nc in ncs], 1).astype(np.int32)
    mask = (rng.uniform(size=(B, T, M)) < 0.7).astype(np.uint8)
    mask[:, :, :6] = 1
    ind[0, 0, 1] = ind[0, 0, 0]                                               # two slots on one (cell, class) (task 0 has one class)
    ind[0, 1, 1], cat[0, 1, 0], cat[0, 1, 1] = ind[0, 1, 0], 0, 1             # two slots on one cell, different classes
    ind[1, 1, 2], cat[1, 1, 2] = ind[1, 1, 1], cat[1, 1, 1]                   # and a same-class pair in another task
    ind[1, 1, 3], ind[1, 1, 4] = 5, 300
    head[1, 5 // W, 5 % W, offs[1]["hm"] + cat[1, 1, 3]] = 30.0               # positives on clipped cells, both sides
    head[1, 300 // W, 300 % W, offs[1]["hm"] + cat[1, 1, 4]] = -30.0
    for b, t, k in ((0, 0, 0), (0, 1, 0), (1, 1, 1)):                         # centre cells as the assigner leaves them
        hm[b, t, cat[b, t, k], ind[b, t, k] // W, ind[b, t, k] % W] = 1.0
    mask[:, 2] = 0                                                            # task 2: no valid slot at all ...
    mask[0, 2, 0], ind[0, 2, 0] = 1, HW                                       # ... but a set mask on the first index past the map
    mask[1, 2, 1], cat[1, 2, 1] = 1, ncs[2]                                   # ... and on the first class past the task's
    mask[0, 0, 5], ind[0, 0, 5] = 1, HW                                       # the same two among valid slots
    mask[1, 1, 5], cat[1, 1, 5] = 1, ncs[1]
    mask[0, 1, 7], ind[0, 1, 7], mask[0, 1, 8], ind[0, 1, 8] = 1, -1, 1, np.iinfo(np.int32).min
    mask[1, 0, 7], cat[1, 0, 7] = 1, -1
    for b, t, k, v in ((0, 0, 9, np.iinfo(np.int32).max), (0, 1, 9, -7), (1, 0, 9, HW * 1000), (1, 2, 9, 1 << 30)):
        mask[b, t, k], ind[b, t, k], cat[b, t, k] = 0, v, 9                   # masked slots with garbage ind and cat
    pr = Problem(head, dict(hm=hm, anno_box=anno, ind=ind, mask=mask, cat=cat), offs, ncs, CODE_WEIGHTS)
    assert pr.want["num_pos"][2] == 0 and pr.want["num_pos"][0] > 6 and pr.want["num_pos"][1] > 6 and len(pr.pad) == 5
    assert (np.abs(head) >= 30).sum() > 500
    return pr


def run(pr, grad=True, out=None, head=None):
    from minddet_amd import det_ops

    h, tg, at = pr.device(head)
    return det_ops.cp_loss(h, tg, at, grad=grad, out=out)


def test_main_shape_equals_the_contract_and_forward_only_equals_forward_with_grad():
    pr = main_problem()
    got = to_np(run(pr))
    check("main", got, pr.want)
    fwd = to_np(run(pr, grad=False))
    assert set(fwd) == {"total", "parts", "num_pos"}
    for k in fwd:
        assert np.array_equal(bits(fwd[k]), bits(got[k])), k
    assert got["num_pos"][2] == 0 and not got["parts"][2, 1:].any() and got["parts"][2, 0] > 0


def test_shape_without_vel_equals_the_contract():
    """fixture `tiles`: W = 72, H = 40 (45 strips), heads without vel: 8 code weights, target columns 0..5, 8, 9"""
    _, _, ncs, kw, tg = fixture_case("tiles")
    B, (W, H) = tg["hm"].shape[0], kw["feature_map_size"]
    offs, Cp = head_layout(ncs, vel=False)
    head = bf16_logits(np.random.default_rng(72), (B, H, W, Cp))
    pr = Problem(head, {k: np.array(tg[k]) for k in KEYS}, offs, ncs, CODE_WEIGHTS[:8])
    assert (W, H) == (72, 40) and pr.want["num_pos"].sum() > 0
    got = to_np(run(pr))
    check("tiles, no vel", got, pr.want)
    assert not got["parts"][:, 10:].any()


def test_column_order_follows_the_offsets():
    """regression channels at the positive cells equal to the (bf16-representable) targets: box_loss == 0 and no regression gradient;
    one head channel moved by 0.5 at one positive cell moves exactly the matching box_loss column (rot sits before vel in the head,
    after it in anno_box)"""
    rng = np.random.default_rng(3)
    B, H, W, M, ncs = 1, 4, 5, 4, [1]
    offs, Cp = head_layout(ncs)
    off = offs[0]
    head = bf16_logits(rng, (B, H, W, Cp), spread=1.0)
    anno = torch.from_numpy(rng.normal(0, 2, (B, 1, M, 10)).astype(np.float32)).to(torch.bfloat16).to(torch.float32).numpy()
    ind = np.array([[[3, 11, 18, 0]]], np.int32)
    mask = np.array([[[1, 1, 1, 0]]], np.uint8)
    cat = np.zeros((B, 1, M), np.int32)
    hm = (rng.uniform(size=(B, 1, 1, H, W)) ** 4).astype(np.float32)
    chans, tcols = cl.columns(off)
    for k in range(3):
        head[0, ind[0, 0, k] // W, ind[0, 0, k] % W, chans] = anno[0, 0, k, tcols]
    targets = dict(hm=hm, anno_box=anno, ind=ind, mask=mask, cat=cat)
    pr = Problem(np.array(head), targets, offs, ncs, CODE_WEIGHTS)
    got = to_np(run(pr))
    reg = np.array(sorted(chans))
    assert not got["parts"][0, 2:].any() and got["parts"][0, 1] == 0 and not got["grad"][..., reg].any() and got["num_pos"][0] == 3
    names = [("reg", 0, 0), ("reg", 1, 1), ("height", 0, 2), ("dim", 0, 3), ("dim", 1, 4), ("dim", 2, 5), ("vel", 0, 6), ("vel", 1, 7),
             ("rot", 0, 8), ("rot", 1, 9)]
    for h, i, col in names:
        moved = np.array(head)
        y, x = 11 // W, 11 % W
        moved[0, y, x, off[h] + i] = float(torch.tensor(float(moved[0, y, x, off[h] + i]) + 0.5).to(torch.bfloat16))
        delta = abs(float(moved[0, y, x, off[h] + i]) - float(head[0, y, x, off[h] + i]))
        g = to_np(run(pr, head=moved))
        box = g["parts"][0, 2:]
        assert delta > 0.25 and np.flatnonzero(box).tolist() == [col], (h, i, box)
        assert abs(box[col] - delta / (3 + 1e-4)) <= 2e-7 * box[col]
        gr = g["grad"][0]
        assert np.argwhere(gr[..., reg] != 0).tolist() == [[y, x, int(np.searchsorted(reg, off[h] + i))]]
        assert abs(gr[y, x, off[h] + i] - WEIGHT * CODE_WEIGHTS[col] / (3 + 1e-4)) <= 2e-7


def test_equal_across_calls_streams_and_the_scratch_pool_with_garbage_filled_outputs():
    from minddet_amd import _lib

    pr = main_problem()
    h, tg, at = pr.device()
    first = to_np(run(pr))

    def garbage():
        out = dict(total=torch.empty((1,), device=DEV), parts=torch.empty((3, 12), device=DEV), num_pos=torch.empty((3,), device=DEV),
                   grad=torch.empty(tuple(h.shape), device=DEV))
        for v in out.values():
            v.view(torch.uint8).fill_(0xFF)
        return out

    filled = garbage()
    assert all(bool((v.view(torch.uint8) == 0xFF).all()) for v in filled.values())
    again = to_np(run(pr, out=filled))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [garbage(), garbage()]
    pool = [garbage(), garbage()]
    fwd = [garbage(), garbage()]
    torch.cuda.synchronize()
    from minddet_amd import det_ops
    for rep in range(2):                                                      # the second round reuses each stream's pool buffer
        for s, o, q, f in zip(streams, outs, pool, fwd):
            with torch.cuda.stream(s):
                det_ops.cp_loss(h, tg, at, grad=True, out=o)
                ops = [h] + [tg[k] for k in KEYS]
                assert _lib.call("md_cp_loss_grad", ops + [q["parts"], q["num_pos"], q["total"], q["grad"]], extra=at) == 0
                assert _lib.call("md_cp_loss", ops + [f["parts"], f["num_pos"], f["total"]], extra=at) == 0
    for o in [again] + [to_np(o) for o in outs + pool]:
        for k in ("total", "parts", "num_pos", "grad"):
            assert np.array_equal(bits(first[k]), bits(o[k])), k               # (a surviving 0xFF byte would differ from `first`)
    for f in fwd:
        f = to_np(f)
        for k in ("total", "parts", "num_pos"):
            assert np.array_equal(bits(first[k]), bits(f[k])), k
    check("main, again", first, pr.want)


def test_autograd_through_center_point_loss():
    from minddet_amd import det_ops

    pr = main_problem()
    h, tg, at = pr.device()
    loss = det_ops.CenterPointLoss(pr.offs, pr.ncs, pr.weight, pr.cw)
    ref = run(pr)
    x = h.clone().requires_grad_(True)
    total, parts, num_pos = det_ops.center_point_loss(x, tg, loss)
    assert total.requires_grad and not parts.requires_grad and not num_pos.requires_grad
    up = torch.tensor([2.5], device=DEV)
    (g,) = torch.autograd.grad(total, x, grad_outputs=up)
    torch.cuda.synchronize()
    assert g.dtype == torch.bfloat16 and g.shape == x.shape
    assert torch.equal(total.detach(), ref["total"]) and torch.equal(parts, ref["parts"]) and torch.equal(num_pos, ref["num_pos"])
    want = (ref["grad"] * 2.5).to(torch.bfloat16)
    assert torch.equal(g.view(torch.int16), want.view(torch.int16)) and bool((g != 0).any())
    y = h.clone().requires_grad_(True)
    (det_ops.center_point_loss(y, tg, loss)[0].sum() * 0.5).backward()
    assert torch.equal(y.grad.view(torch.int16), (ref["grad"] * 0.5).to(torch.bfloat16).view(torch.int16))


def test_production_shape_equals_the_contract():
    """B = 4, the train config: targets from det_ops.cp_assign_targets on 500 seeded objects per sample, the head tensor from
    graphs.CenterHead on random input, through CenterHead.loss"""
    from minddet.models import Config
    from minddet_amd import det_ops, graphs

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_nusc_train.py"))
    tgen = det_ops.CenterPointTargets.from_config(cfg)
    rng = np.random.default_rng(500)
    B, G = 4, tgen.max_objs
    b = np.zeros((B, G, 9), np.float32)
    b[..., 0:2] = rng.uniform(-52.5, 52.5, (B, G, 2))
    b[..., 2] = rng.uniform(-4, 2, (B, G))
    b[..., 3:5] = np.exp(rng.uniform(np.log(0.3), np.log(14.0), (B, G, 2)))
    b[..., 5] = rng.uniform(0.5, 4.0, (B, G))
    b[..., 6:8] = rng.normal(0, 4, (B, G, 2))
    b[..., 8] = rng.uniform(-7.0, 7.0, (B, G))
    c = rng.integers(1, 11, (B, G)).astype(np.int32)
    targets = tgen(torch.from_numpy(b).to(DEV), torch.from_numpy(c).to(DEV))
    head_mod = graphs.CenterHead(**{k: v for k, v in cfg.model["bbox_head"].items() if k != "type"}, **cfg.train_cfg["loss"]).to(DEV)
    W, H = tgen.feature_map_size
    x = torch.from_numpy(rng.normal(0, 1, (B, H, W, head_mod.in_channels)).astype(np.float32)).to(torch.bfloat16).to(DEV)
    head, _ = head_mod(x)
    got = to_np(head_mod.loss(targets, head, grad=True))
    tg = {k: targets[k].cpu().numpy() for k in KEYS}
    hf = head.to(torch.float32).cpu().numpy()
    want = cl.loss(np.nan_to_num(hf), *(tg[k] for k in KEYS), task_offsets=head_mod.task_offsets(), num_classes=head_mod.num_classes,
                   weight=float(np.float32(0.25)), code_weights=[float(np.float32(v)) for v in cfg.train_cfg["loss"]["code_weights"]])
    assert head.shape == (B, H, W, 72) and (H, W) == (128, 128) and want["num_pos"].min() > 100
    check("nusc b4", got, want)
    assert np.array_equal(bits(to_np(head_mod.loss(targets, head))["total"]), bits(got["total"]))
