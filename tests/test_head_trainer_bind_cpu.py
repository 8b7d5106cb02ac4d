"""What the three head trainers share (optim._HeadTrainerBase, optim.bind_range, Adam.adopt) and the trainer hook of graphs.Module,
on CPU packs: the first bind, a rebind around new packs, one Adam per pack beside one Adam over two packs, the config check, and the
order in which Module.to() calls a trainer.  No library call and no GPU: packing and binding are torch on the host."""
import numpy as np
import pytest
import torch

from minddet_amd import graphs, nn_ops, optim

CFG = optim.HeadTrainer.check_config(None)


def _packs(seed):
    """the smallest packs that take every branch: a 1x1 conv 3 -> 5, a 3x3 conv 64 -> 2 in both K orders, a grouped 3x3 pack"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(pw=nn_ops.pack_conv(r(5, 3, 1, 1), bias=r(5)),
                k0=nn_ops.pack_conv(r(2, 64, 3, 3), bias=r(2), pad=1, korder=0),
                k1=nn_ops.pack_conv(r(2, 64, 3, 3), bias=r(2), pad=1, korder=1),
                grouped=nn_ops.pack_conv2d_grouped([(r(2, 64, 3, 3), r(2), None), (r(3, 64, 3, 3), r(3), None)]))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("name", ["pw", "k0", "k1", "grouped"])
def test_first_bind_of_one_pack(name):
    pc = _packs(1)[name]
    w0, b0 = pc.w.clone(), pc.bias.clone()
    opt = optim.bind_range([(pc, "w", "b")], CFG)
    assert opt.param.device.type == "cpu" and opt.n == w0.numel() + b0.numel() and opt.steps == 0
    assert torch.equal(opt.view("w"), w0.to(torch.float32)) and torch.equal(opt.view("b"), b0)            # the master is the widened pack
    assert pc.w.shape == w0.shape and pc.w.dtype == torch.bfloat16 and torch.equal(_bits(pc.w), _bits(w0))
    assert opt.shadow.data_ptr() == pc.w.data_ptr() and opt.shadow.numel() == w0.numel()                  # the conv reads the shadow
    assert pc.bias.data_ptr() == opt.view("b").data_ptr()                                                 # and the master's bias
    assert float(opt.m.abs().sum()) == 0.0 and float(opt.v.abs().sum()) == 0.0
    assert (opt.beta1_power, opt.beta2_power) == (np.float32(1.0), np.float32(1.0))


def test_first_bind_of_two_packs_puts_every_weight_before_every_bias():
    p = _packs(2)
    pc1, pk2 = p["k1"], p["grouped"]
    w1, w2, b1, b2 = pc1.w.clone(), pk2.w.clone(), pc1.bias.clone(), pk2.bias.clone()
    opt = optim.bind_range([(pc1, "w1", "b1"), (pk2, "w2", "b2")], CFG)
    n1, n2 = w1.numel(), w2.numel()
    assert list(opt.slices) == ["w1", "w2", "b1", "b2"]
    assert [opt.slices[k][:2] for k in opt.slices] == [(0, n1), (n1, n1 + n2), (n1 + n2, n1 + n2 + b1.numel()), (n1 + n2 + b1.numel(), opt.n)]
    assert opt.shadow.numel() == n1 + n2 and torch.equal(opt.param[:n1 + n2], torch.cat([w1.reshape(-1), w2.reshape(-1)]).to(torch.float32))
    assert pc1.w.data_ptr() == opt.shadow.data_ptr() and pk2.w.data_ptr() == opt.shadow.data_ptr() + 2 * n1
    assert torch.equal(_bits(pc1.w), _bits(w1)) and torch.equal(_bits(pk2.w), _bits(w2)) and pk2.w.shape == w2.shape
    assert pc1.bias.data_ptr() == opt.view("b1").data_ptr() and pk2.bias.data_ptr() == opt.view("b2").data_ptr()
    assert torch.equal(pc1.bias, b1) and torch.equal(pk2.bias, b2)


def _mutate(opt, seed):
    g = torch.Generator().manual_seed(seed)
    opt.param += 1e-2 * torch.randn(opt.n, generator=g)
    opt.m.copy_(torch.randn(opt.n, generator=g))
    opt.v.copy_(torch.rand(opt.n, generator=g))
    opt.beta1_power, opt.beta2_power, opt.steps = np.float32(0.9) * np.float32(0.85), np.float32(0.999) ** 2, 7


def _carried(new, old):
    return (all(torch.equal(_bits(getattr(new, k)), _bits(getattr(old, k))) and getattr(new, k).data_ptr() != getattr(old, k).data_ptr()
                for k in ("param", "m", "v"))
            and (new.beta1_power, new.beta2_power, new.steps) == (old.beta1_power, old.beta2_power, old.steps)
            and type(new.beta1_power) is np.float32 and type(new.beta2_power) is np.float32)


def test_rebind_carries_master_moments_powers_and_steps_to_new_packs():
    a, b = _packs(3), _packs(4)
    old = optim.bind_range([(a["k1"], "w1", "b1"), (a["grouped"], "w2", "b2")], CFG)
    _mutate(old, 5)
    kept = {k: getattr(old, k).clone() for k in ("param", "m", "v")}
    pc1, pk2 = b["k1"], b["grouped"]
    assert not torch.equal(pc1.w, a["k1"].w)
    new = optim.bind_range([(pc1, "w1", "b1"), (pk2, "w2", "b2")], CFG, old)
    assert _carried(new, old) and new.steps == 7 and new.beta1_power == np.float32(0.9) * np.float32(0.85)
    assert all(torch.equal(getattr(old, k), kept[k]) for k in kept)                                    # the old optimizer keeps its buffers
    n1 = pc1.w.numel()
    assert torch.equal(_bits(pc1.w), _bits(new.view("w1").to(torch.bfloat16))) and torch.equal(_bits(pk2.w), _bits(new.view("w2").to(torch.bfloat16)))
    assert torch.equal(_bits(new.shadow), _bits(new.param[:new.shadow.numel()].to(torch.bfloat16)))
    assert pc1.w.data_ptr() == new.shadow.data_ptr() and pk2.w.data_ptr() == new.shadow.data_ptr() + 2 * n1
    assert pc1.bias.data_ptr() == new.view("b1").data_ptr() and pk2.bias.data_ptr() == new.view("b2").data_ptr()
    assert a["k1"].w.data_ptr() == old.shadow.data_ptr()                                               # and its packs


def test_adopt_is_load_state_of_the_live_buffers():
    a, b = _packs(6), _packs(7)
    old = optim.bind_range([(a["pw"], "w", "b")], CFG)
    _mutate(old, 8)
    x, y = optim.bind_range([(b["pw"], "w", "b")], CFG), optim.bind_range([(_packs(7)["pw"], "w", "b")], CFG)
    x.adopt(old)
    y.load_state(old.state())
    assert _carried(x, old) and _carried(y, old) and torch.equal(_bits(x.shadow), _bits(y.shadow))


class _Owner(graphs.Module):
    def __init__(self, seed):
        for k, v in _packs(seed).items():
            setattr(self, k, v)


class _Trainer(optim._HeadTrainerBase):
    """the base on CPU packs: the constructor without the device check, the ranges given by the test"""
    DEFAULTS = optim.DEFAULT_OPTIMIZER

    def __init__(self, owner, layout):
        self.cfg, self.opts, self.owner, self.layout = self.check_config(None), None, owner, layout
        owner._trainer = self
        self.bind()

    def ranges(self):
        return {r: [(getattr(self.owner, p), wn, bn) for p, wn, bn in packs] for r, packs in self.layout.items()}


def test_two_ranges_and_one_range_over_two_packs_come_out_of_the_same_base():
    two = _Trainer(_Owner(9), dict(head1=[("k1", "w", "b")], head2=[("pw", "w", "b")]))                  # CenterNet's form
    one = _Trainer(_Owner(9), dict(head=[("k1", "w1", "b1"), ("grouped", "w2", "b2")]))                  # CenterPoint's
    assert list(two.opts) == ["head1", "head2"] and list(one.opts) == ["head"] and one.opt is one.opts["head"]
    with pytest.raises(ValueError):
        two.opt
    for name, p in (("head1", "k1"), ("head2", "pw")):
        o, pc = two.opts[name], getattr(two.owner, p)
        assert list(o.slices) == ["w", "b"] and o.shadow.data_ptr() == pc.w.data_ptr() and pc.bias.data_ptr() == o.view("b").data_ptr()
    assert list(one.opt.slices) == ["w1", "w2", "b1", "b2"] and one.opt.n == sum(t.numel() for p in ("k1", "grouped") for t in
                                                                               (getattr(one.owner, p).w, getattr(one.owner, p).bias))
    assert torch.equal(two.opts["head1"].view("w"), one.opt.view("w1"))                                  # the same pack, the same master
    for tr in (two, one):                                                                                # a rebind through the base
        olds = dict(tr.opts)
        for o in olds.values():
            _mutate(o, 10)
        for k, v in _packs(11).items():
            setattr(tr.owner, k, v)
        tr.bind()
        assert list(tr.opts) == list(olds) and all(tr.opts[r] is not olds[r] and _carried(tr.opts[r], olds[r]) for r in olds)
        for r, packs in tr.ranges().items():
            for pc, wn, bn in packs:
                assert torch.equal(_bits(pc.w), _bits(tr.opts[r].view(wn).to(torch.bfloat16))) and pc.bias.data_ptr() == tr.opts[r].view(bn).data_ptr()


def test_host_copy_unpermutes_a_3x3_pack_and_leaves_a_1x1_pack():
    g = torch.Generator().manual_seed(12)
    w = torch.randn(2, 64, 3, 3, generator=g).to(torch.bfloat16).to(torch.float32)
    for korder in (0, 1):
        pc = nn_ops.pack_conv(w, bias=torch.randn(2, generator=g), pad=1, korder=korder)
        opt = optim.bind_range([(pc, "w", "b")], CFG)
        hw, hb = optim._HeadTrainerBase._host(opt, "w", "b", pc)
        assert hw.shape == (pc.w.shape[0], 64, 3, 3) and torch.equal(hw[:2], w) and torch.equal(hb, pc.bias)
    pc = _packs(12)["pw"]
    opt = optim.bind_range([(pc, "w", "b")], CFG)
    assert torch.equal(optim._HeadTrainerBase._host(opt, "w", "b", pc)[0], opt.view("w"))


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the owner was read ({name}) before the config was checked")


@pytest.mark.parametrize("cls,defaults", [(optim.HeadTrainer, optim.DEFAULT_OPTIMIZER), (optim.CenterNetHeadTrainer, optim.CENTERNET_OPTIMIZER),
                                          (optim.CenterPointHeadTrainer, optim.CENTERPOINT_OPTIMIZER)])
def test_config_check(cls, defaults):
    bad = [dict(type="SGD"), dict(type="Adam", momentum=0.9)] + ([dict(type="Adam", max_norm=35.0)] if cls is optim.CenterNetHeadTrainer else [])
    for cfg in bad:
        with pytest.raises(ValueError, match=cls.__name__):
            cls(_Untouchable(), cfg)
    want = {k: v for k, v in defaults.items() if k != "type"}
    assert cls.check_config(None) == want and cls.check_config({}) == want
    assert cls.check_config(dict(type="Adam", weight_decay=0.5, eps=1e-6)) == dict(want, weight_decay=0.5, eps=1e-6)
    assert cls.check_config(dict(max_norm=None))["max_norm"] is None                                     # a refused key may be None
    if cls is not optim.CenterNetHeadTrainer:
        assert cls.check_config(dict(max_norm=35.0))["max_norm"] == 35.0
    with pytest.raises(AssertionError):                                                                  # a good config goes on to the owner
        cls(_Untouchable(), dict(type="Adam"))


class _Recorder:
    def __init__(self, log):
        self.log = log

    def sync_modules(self):
        self.log.append("sync_modules")

    def bind(self):
        self.log.append("bind")


class _Leaf(graphs.Module):
    def __init__(self, log):
        self.log = log

    def _derive(self, device):
        self.log.append("pack child")


class _Parent(graphs.Module):
    def __init__(self, log):
        self.log, self.kids = log, [_Leaf(log), _Leaf(log)]

    def children(self):
        return self.kids

    def _refresh(self):
        self.log.append("refresh")

    def _derive(self, device):
        self.log.append("derive")


def test_module_to_calls_the_trainer_around_the_repack():
    log = []
    trained, plain = _Parent(log), _Parent(log)
    trained._trainer = _Recorder(log)
    assert plain._trainer is None and graphs.Module._trainer is None and trained.kids[0]._trainer is None
    gen0 = graphs.Module.generation
    assert trained.to("cpu") is trained
    assert log == ["sync_modules", "refresh", "pack child", "pack child", "derive", "bind"] and graphs.Module.generation == gen0 + 3
    del log[:]
    plain.to("cpu")
    assert log == ["refresh", "pack child", "pack child", "derive"]
    del log[:]
    trained._derive("cpu")                                                                               # a direct call binds nothing
    assert log == ["derive"]


def test_head_trainer_rule_returns_replaces_and_falls_back():
    made, log = [], []

    class Tr(_Recorder):
        def __init__(self, model, cfg):
            super().__init__(log)
            self.model, self.cfg = model, cfg
            model._trainer = self
            made.append(self)

    m = _Parent(log)
    rederive = lambda: log.append("rederive")
    first = m._head_trainer(Tr, m, None, dict(eps=1.0), rederive)
    assert first.cfg == dict(eps=1.0) and log == [] and m._trainer is first                              # none yet: made with the fallback
    assert m._head_trainer(Tr, m, None, dict(eps=2.0), rederive) is first and len(made) == 1 and log == []
    second = m._head_trainer(Tr, m, dict(eps=3.0), dict(eps=2.0), rederive)                              # an explicit config always replaces
    assert second is not first and second.cfg == dict(eps=3.0) and m._trainer is second and log == ["sync_modules", "rederive"]


def test_lazy_operators_and_train_cfg_live_on_the_instance():
    a, b = _Parent([]), _Parent([])
    built = []
    assert a._lazy("op", lambda: built.append(1) or "A") == "A" and a._lazy("op", lambda: built.append(1) or "B") == "A" and built == [1]
    assert b._lazy("op", lambda: "B") == "B"
    a.train_cfg, b.train_cfg = dict(assigner=1), None
    assert a._train_cfg("assigner") == 1
    for mod, key in ((a, "augment"), (b, "assigner")):
        with pytest.raises(ValueError, match=f"_Parent: train_cfg\\['{key}'\\] is needed for training"):
            mod._train_cfg(key)
