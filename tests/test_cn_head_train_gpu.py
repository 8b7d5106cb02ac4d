"""GPU: graphs.CenterNet.head_trainer -- CenterNet's heads trained on the device with the backbone and the neck frozen
(optim.CenterNetHeadTrainer: head1 -> head2 -> md_cn_loss_grad -> md_conv_bwd_weight -> md_conv1x1_bwd_data -> md_conv_bwd_weight ->
md_adam_step) -- on configs/centernet/centernet_tiny_train.py at B = 2 (a 16 x 24 map, P = 768) with the seeded images and boxes of
tests/test_cn_augment_gpu.py and one fixed draw of the augmentation.

Every condition is on tensors read back, against the float64 judges (tests/convbwd_contract.py, tests/train_contract.py) inside the
header's bounds or bit for bit; the one training condition -- the loss after twenty steps on a fixed batch is lower than before the
first -- has no threshold."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import convbwd_contract as cc, train_contract as tc
from tests.conftest import has_gpu
from tests.test_cn_augment_gpu import dev, tiny_batch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 5e-4                 # train_cfg["lr_config"]["learning_rate"]


def build():
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centernet", "centernet_tiny_train.py"))
    return build_detector(cfg.model, cfg.train_cfg, cfg.test_cfg).to(DEV), cfg


@functools.lru_cache(maxsize=None)
def batch():
    """-> (inp [2,64,96,8] bf16, example): one fixed draw of the augmentation, shared by every test and left unchanged"""
    net, _ = build()
    img, sizes, boxes, classes = tiny_batch()
    draws, colour = net.augment_op().draw(dev(sizes), torch.Generator(device=DEV).manual_seed(6))
    inp, ex = net.train_example(dev(img), dev(sizes), dev(boxes), dev(classes), draws=draws, colour=colour)
    torch.cuda.synchronize()
    assert float(ex["reg_mask"].sum()) >= 2
    return inp, ex


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int16 if t.element_size() == 2 else torch.int32).numpy()


def split(opt, of):
    """an Adam's flat buffer -> (w [rows,kpad], b [rows]) numpy"""
    return getattr(opt, of)[opt.slices["w"][0]:opt.slices["w"][1]].view(opt.slices["w"][2]).cpu().numpy(), opt.view("b", of).cpu().numpy()


def test_one_step_equals_the_contracts():
    net, cfg = build()
    inp, ex = batch()
    tr = net.head_trainer()
    assert tr is net.head_trainer() and tr.cfg["eps"] == cfg.train_cfg["optimizer"]["eps"] == 1e-7 and tr.cfg["weight_decay"] == 0.0
    assert tr.cfg["grad_scale"] == 1.0 and tr.cfg["max_norm"] is None
    pc1, pc2, o1, o2 = net.head1.packed, net.head2.packed, tr.opts["head1"], tr.opts["head2"]
    assert (pc1.cin, pc1.cout, pc1.kh, pc1.korder, tuple(pc1.w.shape)) == (64, 192, 3, 1, (256, 576)) and (pc2.cin, pc2.cout, net.n_out) == (192, 16, 9)
    blocks = tr.blocks()
    assert blocks == [(0, 5, 0, 64), (5, 2, 64, 64), (7, 2, 128, 64)]
    for pc, opt in ((pc1, o1), (pc2, o2)):
        rows, kpad = pc.w.shape
        assert opt.n == rows * kpad + rows and pc.bias.data_ptr() == opt.view("b").data_ptr() and opt.shadow.data_ptr() == pc.w.data_ptr()
        assert np.array_equal(opt.view("w").cpu().numpy(), pc.w.float().cpu().numpy()) and not opt.m.any() and not opt.v.any()
    before = {n: {k: getattr(o, k).cpu().numpy().copy() for k in ("param", "m", "v")} for n, o in tr.opts.items()}
    w2_read = pc2.w.float().cpu().numpy().copy()                                 # the weights the step's forward pass and data gradient read
    plain = net.loss(inp, ex, grad=True)
    out = tr.train_step(inp, ex, lr=LR, beta1=0.9)
    torch.cuda.synchronize()
    for k in ("total", "parts", "num_pos", "grad", "head"):                       # the step reports the loss before the update
        assert np.array_equal(bits(out[k]), bits(plain[k])), k

    x, h, g, dh = out["x"].float().cpu().numpy(), out["h"].float().cpu().numpy(), out["grad"].cpu().numpy(), out["dh"].cpu().numpy()
    assert x.shape == (2, 16, 24, 64) and h.shape == (2, 16, 24, 192) and g.shape == (2, 16, 24, 16) and dh.shape == h.shape and (h >= 0).all()
    P = 2 * 16 * 24

    def inside(name, got, want, bound, live):
        err = np.abs(got.astype(np.float64) - want)
        print(f"cn head step[{name}]: {int(live.sum())} live elements, worst error / bound {float((err[live] / bound[live]).max()):.3e}")
        assert np.isfinite(got).all() and (err <= bound).all(), name
        assert (got[~live].view(np.uint32) == 0).all(), name                      # +0.0 wherever nothing is summed

    # head2: the 1x1 weight gradient inside the three blocks
    dw2, db2 = split(o2, "grad")
    want2 = cc.wgrad_kxk(h, g, 192, 9, kernel=1, blocks=blocks, rows=dw2.shape[0], kpad=dw2.shape[1])
    assert want2["live"].sum() == 9 * 64
    inside("dw2", dw2, want2["dw"], tc.wgrad_bound(P, want2["absdw"]), want2["absdw"] > 0)
    inside("db2", db2, want2["db"], tc.wgrad_bound(P, want2["absdb"]), want2["absdb"] > 0)
    assert (want2["absdw"] > 0).sum() >= 0.5 * 9 * 64 and (want2["absdb"] > 0).sum() == 9
    # the data gradient through head2 and the ReLU of head1
    wantd = cc.dgrad_1x1(g, w2_read, 192, 9, act=h)
    inside("dh", dh, wantd["dx"], cc.dgrad_bound(9, wantd["absdx"]), wantd["absdx"] > 0)
    assert np.array_equal(wantd["keep"], h > 0) and 0.05 < wantd["keep"].mean() < 0.95
    # head1: the 3x3 weight gradient from the device's dh, in the pack's column order
    dw1, db1 = split(o1, "grad")
    want1 = cc.wgrad_kxk(x, dh, 64, 192, kernel=3, korder=pc1.korder, rows=dw1.shape[0], kpad=dw1.shape[1])
    inside("dw1", dw1, want1["dw"], tc.wgrad_bound(P, want1["absdw"]), want1["absdw"] > 0)
    inside("db1", db1, want1["db"], tc.wgrad_bound(P, want1["absdb"]), want1["absdb"] > 0)
    assert (want1["absdw"] > 0).sum() >= 0.5 * 192 * 576

    # Adam on the device's gradient: the contract, element for element
    b1p, b2p = float(np.float32(0.9)), float(np.float32(0.999))
    for name, opt, pc in (("head1", o1, pc1), ("head2", o2, pc2)):
        assert (float(opt.beta1_power), float(opt.beta2_power), opt.steps) == (b1p, b2p, 1)
        grad = opt.grad.cpu().numpy()
        new = tc.adam(grad, before[name]["param"], before[name]["m"], before[name]["v"], lr=LR, beta1=0.9, beta2=0.999, beta1_power=b1p, beta2_power=b2p,
                      eps=1e-7, weight_decay=0.0)
        for k, want in zip(("param", "m", "v"), new):
            apart = tc.ulps_apart(getattr(opt, k).cpu().numpy(), want)
            print(f"cn head step[{name}.{k}]: {int((apart > 0).sum())} of {opt.n} differ, worst {int(apart.max())} ulp")
            assert int((apart > 0).sum()) == 0, (name, k)
        master = opt.view("w").cpu().numpy()
        assert (opt.param.cpu().numpy() != before[name]["param"]).sum() >= 0.5 * np.count_nonzero(grad)
        assert np.array_equal(bits(pc.w).view(np.uint16).reshape(-1), tc.bf16_bits(master.reshape(-1)))      # the pack the conv reads = bf16 of the master


def test_three_steps_keep_head2_block_diagonal_and_the_next_forward_runs_on_the_new_weights():
    from minddet_amd import nn_ops, optim

    net, _ = build()
    inp, ex = batch()
    tr = net.head_trainer()
    old_head = bits(net.features(inp))
    for _ in range(3):
        tr.train_step(inp, ex, lr=LR)
    pc2, o2 = net.head2.packed, tr.opts["head2"]
    live = np.zeros(tuple(pc2.w.shape), bool)
    for r0, nr, c0, nc in tr.blocks():
        live[r0:r0 + nr, c0:c0 + nc] = True
    for of in ("param", "m", "v"):
        w, b = split(o2, of)
        assert (w[~live].view(np.uint32) == 0).all() and (b[9:].view(np.uint32) == 0).all() and np.count_nonzero(w[live]) >= 0.5 * live.sum(), of
    assert (bits(pc2.w).view(np.uint16)[~live] == 0).all()
    # features() reads the trained packs: the same bytes as the two convs on fresh packs of the masters
    x = net.backbone(inp)[-1]
    for m in net.neck:
        x = m(x)
    o1, pc1 = tr.opts["head1"], net.head1.packed
    w1 = o1.view("w").cpu()[:192, optim.pack_columns(pc1).reshape(-1)].reshape(192, 3, 3, 64).permute(0, 3, 1, 2).contiguous()
    fresh1 = nn_ops.pack_conv(w1, bias=o1.view("b").cpu()[:192].clone(), pad=1, relu=True).to(DEV)
    fresh2 = nn_ops.pack_conv(o2.view("w").cpu()[:9].reshape(9, 192, 1, 1).clone(), bias=o2.view("b").cpu()[:9].clone()).to(DEV)
    assert fresh1.korder == pc1.korder and np.array_equal(bits(fresh1.w), bits(pc1.w)) and np.array_equal(bits(fresh2.w), bits(pc2.w))
    want = nn_ops.conv2d(nn_ops.conv2d(x, fresh1), fresh2)
    got = bits(net.features(inp))
    assert np.array_equal(got, bits(want)) and not np.array_equal(got, old_head)
    det = net.forward(inp)                                                        # inference on the trained heads
    torch.cuda.synchronize()
    assert det.shape[0] == 2


def test_to_keeps_the_trained_heads_and_a_replaced_trainer_starts_fresh():
    net, _ = build()
    inp, ex = batch()
    tr = net.head_trainer()
    for _ in range(3):
        tr.train_step(inp, ex, lr=LR)
    head = bits(net.features(inp))
    state = {n: [bits(getattr(o, k)).copy() for k in ("param", "m", "v")] for n, o in tr.opts.items()}
    powers = {n: (o.beta1_power, o.beta2_power) for n, o in tr.opts.items()}
    old_packs = (net.head1.packed, net.head2.packed)
    net.to(DEV)                                                                   # sync_modules, fuse_heads, a repack of everything, bind
    assert net.head_trainer() is tr and net.head1.packed is not old_packs[0] and net.head2.packed is not old_packs[1]
    for n, pc in (("head1", net.head1.packed), ("head2", net.head2.packed)):
        o = tr.opts[n]
        assert o.shadow.data_ptr() == pc.w.data_ptr() and pc.bias.data_ptr() == o.view("b").data_ptr() and o.steps == 3
        assert (o.beta1_power, o.beta2_power) == powers[n]
        assert all(np.array_equal(a, bits(getattr(o, k))) for a, k in zip(state[n], ("param", "m", "v"))), n
    assert np.array_equal(bits(net.features(inp)), head)
    # the per-head modules hold the trained weights (what weights.py exports)
    w2 = tr.opts["head2"].view("w").cpu()
    assert torch.equal(net.heads["wh"][1].weight.reshape(2, 64), w2[5:7, 64:128]) and torch.equal(net.heads["hm"][0].bias, tr.opts["head1"].view("b").cpu()[:64])
    a = tr.train_step(inp, ex, lr=LR)
    assert tr.opts["head1"].steps == 4 and not np.array_equal(bits(net.features(inp)), head) and np.isfinite(float(a["total"].cpu()[0]))

    # a call with a config replaces the trainer: the weights stay, the moments and the powers start again
    head = bits(net.features(inp))
    new = net.head_trainer(dict(type="Adam", eps=1e-7, weight_decay=0.0))
    assert new is not tr and net.head_trainer() is new
    assert np.array_equal(bits(net.features(inp)), head)
    for o in new.opts.values():
        assert o.steps == 0 and float(o.beta1_power) == 1.0 and not o.m.any() and not o.v.any()
    new.train_step(inp, ex, lr=LR)
    torch.cuda.synchronize()                                                      # no kernel of a step outlives its test
    assert new.opts["head2"].steps == 1 and tr.opts["head2"].steps == 4


def test_twenty_steps_lower_the_loss_and_two_models_repeat_bit_for_bit():
    inp, ex = batch()
    net, cfg = build()
    tr = net.head_trainer()
    lr = cfg.train_cfg["lr_config"]["learning_rate"]
    first = float(net.loss(inp, ex)["total"].cpu()[0])
    totals = [tr.train_step(inp, ex, lr=lr)["total"] for _ in range(20)]
    last = float(net.loss(inp, ex)["total"].cpu()[0])
    assert float(totals[0].cpu()[0]) == first
    print(f"cn head training: total {first:.6f} before the first step, {last:.6f} after the twentieth (ratio {last / first:.4f})")
    assert last < first

    runs = []
    for _ in range(2):
        m, _ = build()
        t = m.head_trainer()
        for _ in range(5):
            t.train_step(inp, ex, lr=lr, beta1=0.9)
        torch.cuda.synchronize()
        runs.append([bits(getattr(o, k)).copy() for o in t.opts.values() for k in ("param", "m", "v")] +
                    [bits(m.head1.packed.w).copy(), bits(m.head2.packed.w).copy(), bits(m.features(inp)).copy()])
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
