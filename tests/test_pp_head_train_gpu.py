"""GPU: graphs.PointPillarsNet.head_trainer -- the KITTI head trained on the device with the neck frozen (optim.HeadTrainer: neck -> head ->
md_pp_loss_grad -> md_conv1x1_bwd_weight -> md_adam_step) -- on configs/pointpillars/pointpillars_tiny_train.py at B = 2 with a seeded
pseudo-image and targets from det_ops.assign_targets_batch (five boxes per sample on top of anchors: positives in both samples).

Every condition is on tensors read back, against the float64 contracts (tests/train_contract.py) or bit for bit; the one training
condition -- the loss after twenty steps on a fixed batch is lower than before the first -- has no threshold."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import train_contract as tc
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 2


def build():
    from minddet.models import Config
    from minddet_amd.registry import build_detector

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "pointpillars", "pointpillars_tiny_train.py"))
    return build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).to(DEV), cfg


@functools.lru_cache(maxsize=None)
def batch():
    """-> (pseudo_image [2,32,48,64] bf16, example) for a model of the config (the anchors depend on the config alone)"""
    from minddet_amd import det_ops

    net, cfg = build()
    g = torch.Generator().manual_seed(3)
    canvas = (torch.randn((B, 32, 48, 64), generator=g) * (torch.rand((B, 32, 48, 1), generator=g) < 0.3)).to(torch.bfloat16).to(DEV)
    rng = np.random.default_rng(4)
    boxes, classes = [], []
    for b in range(B):
        pick = torch.from_numpy(rng.choice(net.anchors.shape[0], 5, replace=False)).to(DEV)
        gt = net.anchors[pick].clone()
        gt[:, :2] += 0.03
        boxes.append(gt)
        classes.append(torch.from_numpy(rng.integers(1, 3, 5).astype(np.int32)).to(DEV))
    a = cfg.train_cfg["assigner"]
    labels, reg, _, _ = det_ops.assign_targets_batch(net.anchors, boxes, classes, a["matched_threshold"], a["unmatched_threshold"])
    assert ((labels > 0).sum(1) >= 1).all()
    return canvas, dict(labels=labels, reg_targets=reg)


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int16 if t.element_size() == 2 else torch.int32).numpy()


def test_one_step_equals_the_contracts():
    net, cfg = build()
    canvas, example = batch()
    tr = net.head_trainer()
    assert tr is net.head_trainer() and tr.cfg["weight_decay"] == cfg.train_cfg["optimizer"]["weight_decay"] == 1e-4 and tr.cfg["max_norm"] is None
    pc, opt = net.bbox_head._merged, tr.opt
    rows, kpad = pc.w.shape
    assert (rows, kpad, pc.cin, pc.cout, net.bbox_head.head_channels) == (64, 64, 48, 48, 44) and opt.n == rows * kpad + rows
    assert pc.bias.data_ptr() == opt.view("b").data_ptr() and opt.shadow.data_ptr() == pc.w.data_ptr()
    before = {k: getattr(opt, k).cpu().numpy().copy() for k in ("param", "m", "v")}
    assert np.array_equal(before["param"][:rows * kpad], pc.w.float().cpu().numpy().reshape(-1)) and not before["m"].any() and not before["v"].any()
    plain = net.loss(canvas, example, grad=True)
    out = tr.train_step(canvas, example, lr=1e-3, beta1=0.9)
    torch.cuda.synchronize()
    for k in ("total", "parts", "num_pos", "grad"):                               # the step reports the loss before the update
        assert np.array_equal(bits(out[k]), bits(plain[k])), k

    feat, grad = out["neck"].float().cpu().numpy(), out["grad"].cpu().numpy()
    P = B * feat.shape[1] * feat.shape[2]
    want = tc.wgrad(feat, grad, pc.cin, pc.cout, rows=rows, kpad=kpad)
    g = opt.grad.cpu().numpy()
    dw, db = g[:rows * kpad].reshape(rows, kpad).astype(np.float64), g[rows * kpad:].astype(np.float64)
    ew, eb = np.abs(dw - want["dw"]), np.abs(db - want["db"])
    live = want["absdw"] > 0
    print(f"head step: P {P}, L {tc.chain_length(P)}, worst error / bound dw {float((ew[live] / tc.wgrad_bound(P, want['absdw'])[live]).max()):.3e}")
    pad = np.ones((rows, kpad), bool)                  # rows from 44 on (no conv owns them: their head gradient is zero) and columns from 48 on
    pad[:44, :48] = False
    assert not live[pad].any() and live.sum() >= 0.5 * 44 * 48                    # (a neck channel that is dead on this batch is not live either)
    assert (ew <= tc.wgrad_bound(P, want["absdw"])).all() and (eb <= tc.wgrad_bound(P, want["absdb"])).all()
    assert (g.view(np.uint32)[:rows * kpad].reshape(rows, kpad)[pad] == 0).all() and (g.view(np.uint32)[rows * kpad + 44:] == 0).all()

    b1p, b2p = float(np.float32(0.9)), float(np.float32(0.999))
    assert (float(opt.beta1_power), float(opt.beta2_power), opt.steps) == (b1p, b2p, 1)
    new = tc.adam(g, before["param"], before["m"], before["v"], lr=1e-3, beta1=0.9, beta2=0.999, beta1_power=b1p, beta2_power=b2p, eps=1e-8,
                  weight_decay=1e-4)
    for name, a, b in zip(("param", "m", "v"), (opt.param, opt.m, opt.v), new):
        apart = tc.ulps_apart(a.cpu().numpy(), b)
        print(f"head step[{name}]: {int((apart > 0).sum())} of {opt.n} differ, worst {int(apart.max())} ulp")
        assert apart.max() <= 1 and int((apart > 0).sum()) * 10000 <= opt.n, name
    master = opt.param.cpu().numpy()
    assert (master != before["param"]).sum() >= live.sum()
    assert not master[:rows * kpad].reshape(rows, kpad)[pad].any() and not master[rows * kpad + 44:].any()   # the pack's padding stays zero
    assert np.array_equal(bits(pc.w).view(np.uint16).reshape(-1), tc.bf16_bits(master[:rows * kpad]))      # the pack the conv reads = bf16 of the master


def test_the_next_forward_runs_on_the_new_weights():
    from minddet_amd import nn_ops

    net, _ = build()
    canvas, example = batch()
    tr = net.head_trainer()
    old_head = bits(net.loss(canvas, example)["head"])
    for _ in range(2):
        tr.train_step(canvas, example, lr=1e-3)
    rows, kpad = net.bbox_head._merged.w.shape
    w = tr.opt.view("w").clone()[:44, :48].reshape(44, 48, 1, 1)
    fresh = nn_ops.pack_conv(w, bias=tr.opt.view("b").clone()[:44]).to(DEV)                                # a fresh pack of the master
    assert tuple(fresh.w.shape) == (rows, kpad)
    out = net.loss(canvas, example)
    want = nn_ops.conv2d(net.neck(canvas), fresh)
    torch.cuda.synchronize()
    assert np.array_equal(bits(out["head"]), bits(want)) and not np.array_equal(bits(out["head"]), old_head)
    dets, count = net.forward(canvas)                                                                    # inference on the trained head
    assert dets.shape[0] == B and count.shape == (B,)


def test_twenty_steps_lower_the_loss_and_runs_repeat_bit_for_bit():
    net, _ = build()
    canvas, example = batch()
    tr = net.head_trainer()
    start = tr.opt.state()
    first = float(net.loss(canvas, example)["total"].cpu()[0])
    totals = [tr.train_step(canvas, example, lr=1e-3)["total"] for _ in range(20)]
    last = float(net.loss(canvas, example)["total"].cpu()[0])
    assert float(totals[0].cpu()[0]) == first
    print(f"head training: total {first:.6f} before the first step, {last:.6f} after the twentieth (ratio {last / first:.4f})")
    assert last < first

    runs = []
    for _ in range(2):
        tr.opt.load_state(start)
        for _ in range(5):
            tr.train_step(canvas, example, lr=1e-3, beta1=0.9)
        torch.cuda.synchronize()
        runs.append([bits(getattr(tr.opt, k)).copy() for k in ("param", "m", "v")] + [bits(net.bbox_head._merged.w).copy()])
        assert tr.opt.steps == 5
    assert all(np.array_equal(a, b) for a, b in zip(*runs))


def test_sync_modules_repack_and_to_keep_the_trained_head():
    from minddet_amd import graphs, nn_ops

    net, _ = build()
    canvas, example = batch()
    tr = net.head_trainer()
    for _ in range(3):
        tr.train_step(canvas, example, lr=1e-3)
    feat = net.neck(canvas)
    head = bits(net.bbox_head(feat))
    tr.sync_modules()
    rebuilt = graphs.merged_conv(net.bbox_head.children(), DEV)                                          # a model rebuilt from the three ConvModules
    assert np.array_equal(bits(nn_ops.conv2d(feat, rebuilt)), head)
    assert np.array_equal(bits(rebuilt.w), bits(net.bbox_head._merged.w)) and np.array_equal(bits(rebuilt.bias), bits(net.bbox_head._merged.bias))
    # a later to() repacks everything: the trainer follows the new pack with its master, moments and powers
    state = [bits(getattr(tr.opt, k)).copy() for k in ("param", "m", "v")]
    old_pack = net.bbox_head._merged
    net.to(DEV)
    assert net.head_trainer() is tr and net.bbox_head._merged is not old_pack and tr.opt.shadow.data_ptr() == net.bbox_head._merged.w.data_ptr()
    assert net.bbox_head._merged.bias.data_ptr() == tr.opt.view("b").data_ptr() and tr.opt.steps == 3
    assert all(np.array_equal(a, bits(getattr(tr.opt, k))) for a, k in zip(state, ("param", "m", "v")))
    assert np.array_equal(bits(net.bbox_head(net.neck(canvas))), head)
    a = tr.train_step(canvas, example, lr=1e-3)
    assert tr.opt.steps == 4 and not np.array_equal(bits(net.bbox_head(net.neck(canvas))), head) and np.isfinite(float(a["total"].cpu()[0]))


def test_a_trainer_on_one_instance_leaves_another_untouched():
    net, _ = build()
    other, _ = build()
    canvas, example = batch()
    before = [bits(t).copy() for t in other.forward(canvas)]
    same = [bits(t) for t in net.forward(canvas)]
    assert all(np.array_equal(a, b) for a, b in zip(before, same))                                       # the same seed builds the same model
    tr = net.head_trainer(dict(type="Adam", weight_decay=0.0, max_norm=35.0))                            # (CenterPoint's form: the clip, a per-step beta1)
    assert tr.cfg["max_norm"] == 35.0
    for beta1 in (0.95, 0.94, 0.93):
        tr.train_step(canvas, example, lr=1e-3, beta1=beta1)
    after = [bits(t) for t in other.forward(canvas)]
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert other.bbox_head._trainer is None and float(tr.opt.beta1_power) == float(np.float32(0.95) * np.float32(0.94) * np.float32(0.93))
    assert not np.array_equal(bits(net.bbox_head._merged.w), bits(other.bbox_head._merged.w))
