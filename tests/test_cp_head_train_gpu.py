"""GPU: graphs.CenterHead.head_trainer -- every SepHead branch of CenterPoint's head trained on the device with the neck and the shared
conv frozen (optim.CenterPointHeadTrainer: merged first convs -> md_conv2d_grouped -> md_cp_loss_grad -> md_conv2d_grouped_bwd_weight ->
md_conv2d_grouped_bwd_data -> md_conv_bwd_weight in chunks of 256 output channels -> md_grad_sumsq -> md_adam_step over ONE flat range) --
on configs/centerpoint/centerpoint_pp_tiny_head_train.py at B = 2 (two tasks, 12 branches, a 16 x 16 head, P = 512) with a seeded
pseudo-image and seeded boxes.

Every condition is on tensors read back, against the float64 judges (tests/groupedbwd_contract.py, tests/convbwd_contract.py,
tests/train_contract.py) inside the headers' bounds or bit for bit; the one training condition -- the loss after twenty OneCycle steps on
a fixed batch is lower than before the first -- has no threshold."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import convbwd_contract as cc, groupedbwd_contract as gc, train_contract as tc
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, P, BRANCHES = 2, 2 * 16 * 16, 12


def config(name="centerpoint_pp_tiny_head_train"):
    from minddet.models import Config

    return Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", f"{name}.py"))


def build():
    from minddet.models import build_detector

    cfg = config()
    return build_detector(dict(cfg.model), dict(cfg.train_cfg), cfg.test_cfg).to(DEV), cfg


@functools.lru_cache(maxsize=None)
def batch():
    """-> (pseudo_image [2,64,64,64] bf16, example): seeded, shared by every test and left unchanged"""
    from minddet_amd import det_ops

    cfg = config()
    rng = np.random.default_rng(25)
    G = 6
    boxes = np.zeros((B, G, 9), np.float32)
    boxes[..., 0:2] = rng.uniform(-6.0, 6.0, (B, G, 2))
    boxes[..., 2] = rng.uniform(-2, 0, (B, G))
    boxes[..., 3:5] = np.exp(rng.uniform(np.log(0.4), np.log(4.0), (B, G, 2)))
    boxes[..., 5] = rng.uniform(0.5, 2.0, (B, G))
    boxes[..., 6:8] = rng.normal(0, 2, (B, G, 2))
    boxes[..., 8] = rng.uniform(-3.0, 3.0, (B, G))
    classes = np.array([[1, 2, 3, 1, 2, 0], [3, 1, 1, 2, 3, 2]], np.int32)
    ex = det_ops.CenterPointTargets(cfg.train_cfg["assigner"], cfg.voxel_generator)(torch.from_numpy(boxes).to(DEV), torch.from_numpy(classes).to(DEV))
    canvas = np.where(rng.uniform(size=(B, 64, 64, 1)) < 0.3, np.maximum(rng.normal(0, 1, (B, 64, 64, 64)), 0), 0).astype(np.float32)
    torch.cuda.synchronize()
    return torch.from_numpy(canvas).to(torch.bfloat16).to(DEV), ex


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int16 if t.element_size() == 2 else torch.int32).numpy()


def head_bits(head):
    """the 23 channels the grouped conv writes (channel 23 of the 24 is never written)"""
    return bits(head[..., :23]).copy()


def state(opt):
    return [bits(getattr(opt, k)).copy() for k in ("param", "m", "v")]


@pytest.mark.parametrize("max_norm", [35.0, 0.01], ids=["max_norm 35", "max_norm 0.01 (the clip acts)"])
def test_one_step_equals_the_contracts(max_norm):
    net, cfg = build()
    pi, ex = batch()
    head = net.bbox_head
    if max_norm == 35.0:
        tr = net.head_trainer()
        assert tr.cfg == dict(beta2=0.999, eps=1e-8, weight_decay=0.01, max_norm=35.0, grad_scale=1.0) and cfg.train_cfg["optimizer"]["max_norm"] == 35.0
    else:
        tr = net.head_trainer(dict(type="Adam", weight_decay=0.01, max_norm=max_norm))
    assert tr is net.head_trainer() is head.head_trainer() is head._trainer
    pc1, pk2, opt = head._first, head._second, tr.opt
    assert (pc1.cin, pc1.cout, pc1.kh, pc1.korder, tuple(pc1.w.shape)) == (64, 64 * BRANCHES, 3, 1, (768, 576))
    assert (pk2.groups, pk2.k, tuple(pk2.w.shape), sum(pk2.couts)) == (BRANCHES, 3, (23, 576), 23) and pk2.couts == [2, 1, 3, 2, 2, 1, 2, 1, 3, 2, 2, 2]
    n1, n2 = 768 * 576, 23 * 576
    # one flat range [w_first | w_second | b_first | b_second]; the packs read the one shadow and the master's bias slices
    assert list(opt.slices) == ["w1", "w2", "b1", "b2"] and opt.n == n1 + n2 + 768 + 23 and opt.shadow.numel() == n1 + n2
    assert pc1.w.data_ptr() == opt.shadow.data_ptr() and pk2.w.data_ptr() == opt.shadow.data_ptr() + 2 * n1
    assert pc1.bias.data_ptr() == opt.view("b1").data_ptr() and pk2.bias.data_ptr() == opt.view("b2").data_ptr()
    assert np.array_equal(opt.view("w1").cpu().numpy(), pc1.w.float().cpu().numpy()) and not opt.m.any() and not opt.v.any()
    before = {k: getattr(opt, k).cpu().numpy().copy() for k in ("param", "m", "v")}
    w2_read = pk2.w.float().cpu().numpy().copy()                                 # the weights the step's forward pass and data gradient read
    plain = net.loss(pi, ex, grad=True)
    lr, beta1 = 1e-3, 0.95
    out = tr.train_step(net.neck(pi), ex, lr=lr, beta1=beta1)
    torch.cuda.synchronize()
    for k in ("total", "parts", "num_pos", "grad"):                               # the step reports the loss before the update
        assert np.array_equal(bits(out[k]), bits(plain[k])), k
    sh, mid, g, dmid = (out[k].float().cpu().numpy() for k in ("shared", "mid", "grad", "dmid"))
    assert sh.shape == (B, 16, 16, 64) and mid.shape == (B, 16, 16, 768) and g.shape == (B, 16, 16, 24) and dmid.shape == mid.shape and (mid >= 0).all()
    L = tc.chain_length(P)

    def inside(name, got, want, bound, live):
        err = np.abs(got.astype(np.float64) - want)
        print(f"cp head step[{name}]: {int(live.sum())} live elements, worst error / bound {float((err[live] / bound[live]).max()):.3e}")
        assert np.isfinite(got).all() and (err <= bound).all(), name
        assert (got[~live].view(np.uint32) == 0).all(), name                      # +0.0 wherever nothing is summed

    # the grouped conv: the weight gradient of every branch's last conv from the device's mid and g
    tb = gc.table(3, pk2.couts, pk2.y_offs, pk2.w_rows)
    dw2, db2 = opt.view("w2", "grad").cpu().numpy(), opt.view("b2", "grad").cpu().numpy()
    want2 = gc.wgrad_grouped(mid, g, tb, 23)
    inside("dw2", dw2, want2["dw"], L * 2.0 ** -24 * want2["absdw"], want2["absdw"] > 0)
    inside("db2", db2, want2["db"], L * 2.0 ** -24 * want2["absdb"], want2["absdb"] > 0)
    assert want2["live"].all() and (want2["absdw"] > 0).sum() >= 0.5 * 23 * 576 and (want2["absdb"] > 0).sum() == 23
    # the data gradient through the grouped conv and the ReLU of the first convs
    wantd = gc.dgrad_grouped(g, w2_read, tb, act=mid)
    inside("dmid", dmid, wantd["dx"], gc.dgrad_bound(wantd), wantd["absdx"] > 0)
    assert np.array_equal(wantd["keep"], mid > 0) and 0.05 < wantd["keep"].mean() < 0.95
    # the merged first convs: the 3x3 weight gradient from the device's dmid in three chunks, in the pack's column order
    dw1, db1 = opt.view("w1", "grad").cpu().numpy(), opt.view("b1", "grad").cpu().numpy()
    want1 = cc.wgrad_kxk(sh, dmid, 64, 768, kernel=3, korder=pc1.korder, rows=768, kpad=576)
    inside("dw1", dw1, want1["dw"], L * 2.0 ** -24 * want1["absdw"], want1["absdw"] > 0)
    inside("db1", db1, want1["db"], L * 2.0 ** -24 * want1["absdb"], want1["absdb"] > 0)
    assert (want1["absdw"] > 0).sum() >= 0.5 * 768 * 576

    # Adam with the global-norm clip on the device's gradient and the device's squared norm: the contract, element for element
    b1p, b2p = float(np.float32(beta1)), float(np.float32(0.999))
    assert (float(opt.beta1_power), float(opt.beta2_power), opt.steps) == (b1p, b2p, 1)
    grad, ss = opt.grad.cpu().numpy(), float(opt.sumsq.cpu()[0])
    assert abs(ss - tc.sumsq(grad)) <= 1e-12 * ss
    coef = max_norm / (np.sqrt(ss) + 1e-6)
    print(f"cp head step: gradient norm {np.sqrt(ss):.6f}, max_norm {max_norm}, clip coefficient {coef:.6f}")
    assert max_norm == 35.0 or coef < 1
    new = tc.adam(grad, before["param"], before["m"], before["v"], lr=lr, beta1=beta1, beta2=0.999, beta1_power=b1p, beta2_power=b2p, eps=1e-8,
                  weight_decay=0.01, sumsq=[ss], max_norm=max_norm)
    for k, want in zip(("param", "m", "v"), new):
        apart = tc.ulps_apart(getattr(opt, k).cpu().numpy(), want)
        print(f"cp head step[{k}]: {int((apart > 0).sum())} of {opt.n} differ, worst {int(apart.max())} ulp")
        assert int((apart > 0).sum()) == 0, k
    assert (opt.param.cpu().numpy() != before["param"]).sum() >= 0.5 * np.count_nonzero(grad)
    master = opt.param.cpu().numpy()[:n1 + n2]
    assert np.array_equal(bits(opt.shadow).view(np.uint16), tc.bf16_bits(master))                            # the packs the convs read = bf16 of the master
    assert np.array_equal(bits(pc1.w).reshape(-1), bits(opt.shadow)[:n1]) and np.array_equal(bits(pk2.w).reshape(-1), bits(opt.shadow)[n1:])


def test_to_keeps_the_trained_head_and_two_models_repeat_bit_for_bit():
    pi, ex = batch()
    runs = []
    for _ in range(2):
        net, _ = build()
        tr = net.head_trainer()
        feat = net.neck(pi)
        for i in range(5):
            tr.train_step(feat, ex, lr=1e-3, beta1=0.95 - 0.02 * i)
        torch.cuda.synchronize()
        runs.append(state(tr.opt) + [bits(tr.opt.shadow).copy(), head_bits(net.bbox_head(feat)[0])])
    assert all(np.array_equal(a, b) for a, b in zip(*runs))

    head = net.bbox_head
    before, st, powers = head_bits(head(feat)[0]), state(tr.opt), (tr.opt.beta1_power, tr.opt.beta2_power)
    old = (head._first, head._second)
    net.to(DEV)                                                                   # sync_modules, a repack of everything, bind
    assert net.head_trainer() is tr and head._first is not old[0] and head._second is not old[1]
    o = tr.opt
    assert head._first.w.data_ptr() == o.shadow.data_ptr() and head._second.bias.data_ptr() == o.view("b2").data_ptr() and o.steps == 5
    assert (o.beta1_power, o.beta2_power) == powers and all(np.array_equal(a, b) for a, b in zip(st, state(o)))
    assert np.array_equal(head_bits(head(feat)[0]), before)                            # the head tensor, byte for byte
    # the per-branch modules hold the trained weights (what weights.center_head_state exports) behind a BatchNorm that folds to nothing
    from minddet_amd import nn_ops, optim
    _, _, c1, c2 = head.branches()[7]
    w1 = o.view("w1").cpu()[:, optim.pack_columns(head._first).reshape(-1)].reshape(768, 3, 3, 64).permute(0, 3, 1, 2)
    fw, fb = nn_ops._fold_bn(c1.weight, c1.bias, c1.bn)
    assert torch.equal(fw, w1[7 * 64:8 * 64]) and torch.equal(fb, o.view("b1").cpu()[7 * 64:8 * 64])
    r0 = head._second.w_rows[7]
    assert torch.equal(c2.weight, o.view("w2").cpu()[r0:r0 + c2.cout].reshape(c2.cout, 3, 3, 64).permute(0, 3, 1, 2)) and torch.equal(c2.bias, o.view("b2").cpu()[r0:r0 + c2.cout])
    a = tr.train_step(feat, ex, lr=1e-3, beta1=0.9)
    assert o.steps == 6 and not np.array_equal(head_bits(head(feat)[0]), before) and np.isfinite(float(a["total"].cpu()[0]))
    # a call with a config replaces the trainer: the weights stay, the moments and the powers start again
    before = head_bits(head(feat)[0])
    new = net.head_trainer(dict(type="Adam", weight_decay=0.0, max_norm=None))
    assert new is not tr and net.head_trainer() is new and np.array_equal(head_bits(head(feat)[0]), before)
    assert new.opt.steps == 0 and float(new.opt.beta1_power) == 1.0 and not new.opt.m.any() and not new.opt.v.any()
    new.train_step(feat, ex, lr=1e-3)
    torch.cuda.synchronize()                                                      # no kernel of a step outlives its test
    assert new.opt.steps == 1 and tr.opt.steps == 6


def test_twenty_one_cycle_steps_lower_the_loss():
    from minddet_amd import optim

    pi, ex = batch()
    net, cfg = build()
    c = cfg.train_cfg["lr_config"]
    lrs, moms = optim.OneCycle(20, c["lr_max"], c["div_factor"], c["pct_start"], c["moms"]).get_lr()
    first = float(net.loss(pi, ex)["total"].cpu()[0])
    totals = [net.train_step(pi, ex, float(lrs[i]), float(moms[i]))["total"] for i in range(20)]
    last = float(net.loss(pi, ex)["total"].cpu()[0])
    assert float(totals[0].cpu()[0]) == first
    print(f"cp head training: total {first:.6f} before the first step, {last:.6f} after the twentieth (ratio {last / first:.4f})")
    assert last < first


def test_a_model_without_a_trainer_is_unchanged_by_the_feature():
    """two fresh models from one seed: one never creates a trainer, the other creates one (no step): the same head and detections"""
    pi, _ = batch()
    plain, _ = build()
    other, _ = build()
    tr = other.head_trainer()
    assert plain.bbox_head._trainer is None and tr.opt.steps == 0
    (da, ca), aux_a = plain.forward(pi, return_aux=True)
    (db, cb), aux_b = other.forward(pi, return_aux=True)
    torch.cuda.synchronize()
    assert np.array_equal(bits(aux_a["head"][..., :23]), bits(aux_b["head"][..., :23])) and np.array_equal(bits(aux_a["shared"]), bits(aux_b["shared"]))
    assert np.array_equal(bits(da), bits(db)) and np.array_equal(bits(ca), bits(cb))
    again = plain.forward(pi)
    assert np.array_equal(bits(again[0]), bits(da))


def test_pillar_detector_train_step_from_raw_points():
    from minddet.models import build_detector

    cfg = config("centerpoint_pp_tiny_points_train")
    m = build_detector(dict(cfg.model), dict(cfg.train_cfg), cfg.test_cfg).to(DEV)
    rng = np.random.default_rng(8)
    Bn, G, n = 2, 4, 1500
    boxes = np.zeros((Bn, G, 9), np.float32)
    for b in range(Bn):
        for g in range(G):
            boxes[b, g] = (-4.5 + 3 * g + rng.uniform(-0.2, 0.2), rng.uniform(-3.5, 3.5), -1.0, 0.8, 1.6, 1.5, rng.uniform(-2, 2), rng.uniform(-2, 2),
                           rng.uniform(-3, 3))
    classes, count = np.tile(np.array([[1, 2, 3, 1]], np.int32), (Bn, 1)), np.array([4, 3], np.int32)
    pts = []
    for b in range(Bn):
        inside = boxes[b, rng.integers(0, G, n), :3] + rng.uniform(-0.3, 0.3, (n, 3))
        bg = np.stack([rng.uniform(-6.4, 6.4, n), rng.uniform(-6.4, 6.4, n), rng.uniform(-3, 1, n)], 1)
        xyz = np.where((rng.uniform(size=n) < 0.3)[:, None], inside, bg)
        pts.append(np.concatenate([xyz, rng.uniform(0, 1, (n, 2))], 1).astype(np.float32))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    args = (dev(np.concatenate(pts)), dev(np.arange(Bn + 1, dtype=np.int32) * n), dev(boxes), dev(classes), dev(count))
    draws = m.augment_op().draw(Bn, torch.Generator(device=DEV).manual_seed(3))
    tr = m.head_trainer()
    assert tr is m.detector.head_trainer() and tr.cfg["max_norm"] == 35.0 and tr.cfg["weight_decay"] == 0.01
    w_before = bits(tr.opt.param).copy()
    out = m.train_step(*args, lr=1e-3, beta1=0.95, draws=draws)
    torch.cuda.synchronize()
    total = float(out["total"].cpu()[0])
    assert np.isfinite(total) and total > 0 and float(out["num_pos"].sum()) >= 2 and "example" in out and out["head"].shape[:3] == (Bn, 16, 16)
    assert np.isfinite(tr.opt.param.cpu().numpy()).all() and tr.opt.steps == 1 and not np.array_equal(bits(tr.opt.param), w_before)
    plain = m.train_loss(*args, draws=draws)
    assert np.isfinite(float(plain["total"].cpu()[0])) and float(plain["total"].cpu()[0]) != total
