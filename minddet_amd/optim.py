"""The optimizer side of a training step: the reference's learning-rate schedules on the host (numpy, one array per run) and its Adam
on the device (det_ops.grad_sumsq + det_ops.adam_step, include/minddet_hip_train.h), plus the trainers of the KITTI head, of
CenterNet's heads and of CenterPoint's head.

  OneCycle               centerpoint/det3d_ms/solver/learning_schedules_fastai.py (OneCycle.get_lr: two cosine phases for the rate and
                         for beta1)
  exponential_decay_lr   the schedule pointpillars/train.py:76-93 asks MindSpore for (the function itself is not in the reference)
  multi_epochs_decay_lr  centernet/src/utils.py:501-538 (MultiEpochsDecayLR, the MultiDecay schedule of centernet/default_config.yaml)
  Adam                   centerpoint/det3d_ms/solver/custom_adam.py:590-668 (Adam.construct); max_norm=None is the plain nn.Adam of
                         pointpillars/train.py
  HeadTrainer            graphs.PointPillarsNet.head_trainer(): neck -> head -> md_pp_loss_grad -> md_conv1x1_bwd_weight ->
                         md_grad_sumsq -> md_adam_step on the merged 1x1 heads, the neck frozen
  CenterNetHeadTrainer   graphs.CenterNet.head_trainer(): head1 (3x3 + ReLU) -> head2 (block-diagonal 1x1) -> md_cn_loss_grad ->
                         md_conv_bwd_weight -> md_conv1x1_bwd_data -> md_conv_bwd_weight -> md_adam_step, backbone and neck frozen
  CenterPointHeadTrainer graphs.CenterHead.head_trainer(): merged first convs (3x3 + ReLU) -> md_conv2d_grouped -> md_cp_loss_grad ->
                         md_conv2d_grouped_bwd_weight -> md_conv2d_grouped_bwd_data -> md_conv_bwd_weight (chunked) -> md_grad_sumsq ->
                         md_adam_step over one flat range (the global-norm clip), neck and shared conv frozen

Nothing here reads a device value back."""
import math

import numpy as np
import torch

from . import det_ops


def _annealing_cos(start, end, pct):
    return end + (start - end) / 2 * (np.cos(np.pi * pct) + 1)


class OneCycle:
    """The reference's OneCycle(total_step, lr_max, div_factor, pct_start, moms): the rate rises from lr_max / div_factor to lr_max over
    the first int(pct_start total_step) steps and falls to lr_max / div_factor / 1e4 over the rest, beta1 goes moms[0] -> moms[1] ->
    moms[0], each phase a half cosine of (step - start) / (end - start).  get_lr() -> (lrs, moms), float32 arrays of total_step values,
    equal bit for bit to the reference's (tests/golden/one_cycle_vectors.npz)."""

    def __init__(self, total_step, lr_max, div_factor, pct_start, moms=(0.95, 0.85)):
        self.total_step, self.lr_max, self.div_factor, self.pct_start, self.moms = int(total_step), lr_max, div_factor, pct_start, tuple(moms)
        low = lr_max / div_factor
        cut = int(pct_start * self.total_step)
        if not 0 < cut < self.total_step:
            raise ValueError(f"OneCycle: the second phase starts inside the run, got step {cut} of {self.total_step}")
        # (first step, one past the last, value at the phase's start, at its end)
        self.lr_phases = [(0, cut, low, lr_max), (cut, self.total_step, lr_max, low / 1e4)]
        self.mom_phases = [(0, cut, self.moms[0], self.moms[1]), (cut, self.total_step, self.moms[1], self.moms[0])]

    @staticmethod
    def _at(phases, step):
        start, end, a, b = [ph for ph in phases if step >= ph[0]][-1]
        return _annealing_cos(a, b, (step - start) / (end - start))

    def step(self, step):
        return self._at(self.lr_phases, step), self._at(self.mom_phases, step)

    def get_lr(self):
        vals = [self.step(i) for i in range(self.total_step)]
        return np.array([v[0] for v in vals]).astype(np.float32), np.array([v[1] for v in vals]).astype(np.float32)


def exponential_decay_lr(learning_rate, decay_rate, total_step, step_per_epoch, decay_epoch, is_stair=False):
    """learning_rate decay_rate^(epoch / decay_epoch) per step, epoch = step // step_per_epoch, the exponent floored when is_stair -> a
    list of total_step Python floats.  Unpinned: the reference (pointpillars/train.py:76-93) calls MindSpore's function of this name,
    which is not in its repository; this is that function's documented form, evaluated in float64."""
    if total_step < 1 or step_per_epoch < 1 or decay_epoch < 1:
        raise ValueError("exponential_decay_lr: total_step, step_per_epoch and decay_epoch are positive")
    out = []
    for i in range(int(total_step)):
        e = (i // int(step_per_epoch)) / int(decay_epoch)
        out.append(float(learning_rate) * float(decay_rate) ** (math.floor(e) if is_stair else e))
    return out


def multi_epochs_decay_lr(learning_rate, multi_epochs, steps_per_epoch, factor, total_step):
    """The reference's MultiEpochsDecayLR (centernet/src/utils.py:501-538; CenterNetMultiEpochsDecayLR.construct returns it, its warm-up
    commented out): learning_rate / factor^k at step i, k = the number of multi_epochs whose first step multi_epochs[j] steps_per_epoch
    is <= i -> a list of total_step Python floats, evaluated in float64."""
    if not isinstance(multi_epochs, (list, tuple)):
        raise TypeError("multi_epochs must be list or tuple.")
    if total_step < 1 or steps_per_epoch < 1:
        raise ValueError("multi_epochs_decay_lr: total_step and steps_per_epoch are positive")
    cuts = [float(e) * int(steps_per_epoch) for e in multi_epochs]
    return [float(learning_rate) / float(factor) ** sum(c <= i for c in cuts) for i in range(int(total_step))]


class Adam:
    """The reference's Adam over one flat fp32 range on the device.  `param`, `grad`, `m`, `v` are flat [n] f32 buffers; view(name) is a
    tensor's slice of any of them (`sizes`: ordered {name: shape}).  step(lr, beta1) advances the two running powers as the reference's
    fp32 Parameters do (beta1_power *= beta1, beta2_power *= beta2, before the update) and runs md_grad_sumsq (only with max_norm) and
    md_adam_step once.  max_norm=None: pointpillars/train.py's nn.Adam(weight_decay); max_norm=35 with a per-step beta1 (OneCycle's
    moms): CenterPoint's.  shadow: a bf16 tensor whose first elements mirror param (the packed weights a conv reads)."""

    def __init__(self, sizes, device, beta2=0.999, eps=1e-8, weight_decay=0.0, max_norm=None, grad_scale=1.0, shadow=None):
        self.slices, n = {}, 0
        for name, shape in sizes.items():
            k = int(np.prod(shape))
            self.slices[name] = (n, n + k, tuple(shape))
            n += k
        self.n = n
        self.param, self.grad, self.m, self.v = (torch.zeros((n,), dtype=torch.float32, device=device) for _ in range(4))
        self.sumsq = torch.zeros((1,), dtype=torch.float64, device=device)
        self.beta2, self.eps, self.weight_decay, self.max_norm, self.grad_scale = float(beta2), float(eps), float(weight_decay), max_norm, float(grad_scale)
        self.beta1_power, self.beta2_power = np.float32(1.0), np.float32(1.0)
        self.shadow = shadow
        self.steps = 0

    def view(self, name, of="param"):
        lo, hi, shape = self.slices[name]
        return getattr(self, of)[lo:hi].view(shape)

    def step(self, lr, beta1=0.9):
        self.beta1_power = np.float32(self.beta1_power * np.float32(beta1))
        self.beta2_power = np.float32(self.beta2_power * np.float32(self.beta2))
        clip = self.max_norm is not None
        if clip:
            det_ops.grad_sumsq(self.grad, out=self.sumsq)
        det_ops.adam_step(self.grad, self.param, self.m, self.v, lr=lr, beta1=beta1, beta2=self.beta2, beta1_power=float(self.beta1_power),
                          beta2_power=float(self.beta2_power), eps=self.eps, weight_decay=self.weight_decay,
                          sumsq=self.sumsq if clip else None, max_norm=self.max_norm, grad_scale=self.grad_scale,
                          shadow=None if self.shadow is None else self.shadow.view(-1))
        self.steps += 1

    def state(self):
        """the mutable state, cloned (the device buffers and the two powers): load_state(state()) restores this moment"""
        return dict(param=self.param.clone(), m=self.m.clone(), v=self.v.clone(), beta1_power=self.beta1_power, beta2_power=self.beta2_power,
                    steps=self.steps)

    def load_state(self, st):
        for k in ("param", "m", "v"):
            getattr(self, k).copy_(st[k])           # (from any device)
        self.beta1_power, self.beta2_power, self.steps = np.float32(st["beta1_power"]), np.float32(st["beta2_power"]), int(st["steps"])
        self.refresh_shadow()

    def adopt(self, old):
        """the mutable state of another Adam over the same layout, on any device (a trainer's rebind): load_state without the clone"""
        self.load_state(vars(old))

    def refresh_shadow(self):
        """the fp32 master rounded into the bf16 shadow"""
        if self.shadow is not None:
            self.shadow.view(-1).copy_(self.param[:self.shadow.numel()].to(torch.bfloat16))


def pack_columns(pc):
    """[kh kw, cin] int64: the column of pc.w that holds tap t, input channel i -- the two K orders of nn_ops.pack_conv, col(t, i) of
    include/minddet_hip_convbwd.h"""
    taps, cin = pc.kh * pc.kw, pc.cin
    t, i = torch.meshgrid(torch.arange(taps), torch.arange(cin), indexing="ij")
    if getattr(pc, "korder", 0) == 1:
        return (i // 64) * (taps * 64) + t * 64 + i % 64
    return t * cin + i


def bind_range(packs, cfg, old=None):
    """One Adam (options cfg) around the packs of a range, packs = [(pack, its weight's slice name, its bias's), ...]: the flat fp32
    master is [every pack's w ... | every pack's bias ...] (weights first: the shadow mirrors param[:shadow.numel()]), the shadow one
    fresh bf16 buffer.  old None: the master is the packs widened to fp32; else the master, moments, powers and step count of `old`
    (an Adam of the same layout, on any device) carried over.  Then the packs read the optimizer's memory: every `w` becomes a view
    of the shadow, every `bias` the master's slice, so the forward pass behind a step runs on the new weights with no copy."""
    dev = packs[0][0].w.device
    sizes = {wn: tuple(pc.w.shape) for pc, wn, _ in packs}
    sizes.update({bn: tuple(pc.bias.shape) for pc, _, bn in packs})
    shadow = torch.empty((sum(pc.w.numel() for pc, _, _ in packs),), dtype=torch.bfloat16, device=dev)
    opt = Adam(sizes, dev, shadow=shadow, **cfg)
    if old is None:
        for pc, wn, bn in packs:
            opt.view(wn).copy_(pc.w.to(torch.float32))
            opt.view(bn).copy_(pc.bias)
        opt.refresh_shadow()
    else:
        opt.adopt(old)
    for pc, wn, bn in packs:
        lo, hi, shape = opt.slices[wn]
        pc.w, pc.bias = shadow[lo:hi].view(shape), opt.view(bn)
    return opt


class _HeadTrainerBase:
    """What the head trainers share, everything that is not a model's arithmetic: the optimizer config, the registration with the
    module that owns the packs, the binding of one Adam per range (bind_range) and the host copy of a master.  A subclass names its
    DEFAULTS (the keys an optimizer_cfg may set, `type` must be "Adam") and the keys it REFUSES unless None, and gives
      _attach(model)  keeps what train_step reads of the constructor's first argument -> the owner: the graphs.Module whose to()
                      makes the packs and which holds the trainer as `_trainer` (Module.to: sync_modules() before a repack,
                      bind() after it; Module._head_trainer replaces the trainer)
      ranges()        ordered {range name: [(pack, weight slice name, bias slice name), ...]} of the owner's CURRENT packs
      train_step, and the loops of sync_modules that write the masters into the model's own modules."""
    DEFAULTS, REFUSES = None, ()

    @classmethod
    def check_config(cls, optimizer_cfg):
        """optimizer_cfg over the DEFAULTS -> Adam's options (no `type`); ValueError for what is not built"""
        cfg = dict(cls.DEFAULTS, **dict(optimizer_cfg or {}))
        if cfg.pop("type") != "Adam":
            raise ValueError(f"{cls.__name__}: only the reference's Adam is built")
        bad = sorted(set(cfg) - set(cls.DEFAULTS)) + [k for k in cls.REFUSES if cfg.get(k) is not None]
        if bad:
            raise ValueError(f"{cls.__name__}: optimizer options that are not built: {bad}")
        return cfg

    def __init__(self, model, optimizer_cfg=None):
        self.cfg, self.opts = self.check_config(optimizer_cfg), None       # (raises before the model is touched)
        owner = self._attach(model)
        if any(pc is None or not pc.w.is_cuda for packs in self.ranges().values() for pc, _, _ in packs):
            raise ValueError(f"{type(self).__name__}: move the model to its device first (to(device) makes the packs)")
        owner._trainer = self
        self.bind()

    @property
    def opt(self):
        """the Adam of a trainer with one range"""
        (opt,) = self.opts.values()
        return opt

    def bind(self):
        """(re)build the flat buffers around the owner's current packs; the fp32 masters, the moments, the powers and the step counts
        survive"""
        old = self.opts or {}
        self.opts = {name: bind_range(packs, self.cfg, old.get(name)) for name, packs in self.ranges().items()}

    @staticmethod
    def _host(opt, wname, bname, pc=None):
        """(w, b) of a slice pair on the host; with a nn_ops.pack_conv pack that is not 1x1, w as [rows, cin, kh, kw] (through the
        pack's column map), else as it lies"""
        w, b = opt.view(wname).detach().cpu(), opt.view(bname).detach().cpu()
        if pc is not None and pc.kh * pc.kw > 1:
            w = w[:, pack_columns(pc).reshape(-1)].reshape(w.shape[0], pc.kh, pc.kw, pc.cin).permute(0, 3, 1, 2)
        return w, b


DEFAULT_OPTIMIZER = dict(type="Adam", beta2=0.999, eps=1e-8, weight_decay=1e-4, max_norm=None, grad_scale=1.0)


class HeadTrainer(_HeadTrainerBase):
    """Trains graphs.PPAnchorHead (conv_cls, conv_box, conv_dir_cls as the one merged 1x1 launch) on the device with the neck frozen.
    The flat parameter (`opt`) is the merged pack widened to fp32 followed by its bias; the merged pack's bf16 `w` is the optimizer's
    shadow and the pack's bias IS the master's bias slice, so the forward pass behind a step runs on the new weights with no copy.
    The head owns the trainer (Module.to): a later to() writes the master back into the three ConvModules, repacks, and binds the
    trainer to the new pack with its moments and powers kept.
    optimizer_cfg: train_cfg["optimizer"] (keys of DEFAULT_OPTIMIZER; `type` must be "Adam")."""
    DEFAULTS = DEFAULT_OPTIMIZER

    def _attach(self, net):
        self.net, self.head = net, net.bbox_head
        return self.head

    def ranges(self):
        return dict(head=[(self.head._merged, "w", "b")])

    def train_step(self, pseudo_image, example, lr, beta1=0.9):
        """One step on a batch: pseudo_image [B,H,W,64] bf16, example = dict(labels, reg_targets) of the model's anchors -> the dict of
        PointPillarsNet.loss(grad=True) (the loss BEFORE the update) plus `neck`.  Nothing is read back."""
        net, opt = self.net, self.opt
        feat = net.neck(pseudo_image)
        head = self.head(feat)
        out = net.loss_op()(head, example["labels"], example["reg_targets"], net.anchors, grad=True)
        det_ops.conv1x1_bwd_weight(feat, out["grad"], self.head._merged, out=(opt.view("w", "grad"), opt.view("b", "grad")))
        opt.step(lr, beta1)
        return dict(out, head=head, neck=feat)

    def sync_modules(self):
        """the fp32 master back into conv_cls / conv_box / conv_dir_cls (weight [cout,cin,1,1], bias [cout]), where weights.py and a
        repack read it.  A host copy: for export, not for the step."""
        w, b = self._host(self.opt, "w", "b")
        row = 0
        for mod in self.head.children():
            mod.weight = w[row:row + mod.cout, :mod.cin].reshape(mod.cout, mod.cin, 1, 1).clone()
            mod.bias = b[row:row + mod.cout].clone()
            row += mod.cout


CENTERNET_OPTIMIZER = dict(type="Adam", beta2=0.999, eps=1e-7, weight_decay=0.0, max_norm=None, grad_scale=1.0)


class CenterNetHeadTrainer(_HeadTrainerBase):
    """Trains the heads of graphs.CenterNet (head1: the fused 3x3 conv + ReLU, head2: the block-diagonal 1x1 conv) on the device with
    the backbone and the neck frozen: head1 -> head2 -> md_cn_loss_grad -> md_conv_bwd_weight (head2, inside its three blocks) ->
    md_conv1x1_bwd_data (through head1's ReLU) -> md_conv_bwd_weight (head1, 3x3) -> md_adam_step per pack.
    One Adam per pack (`opts["head1"]`, `opts["head2"]`): the flat parameter is the pack widened to fp32 followed by its bias, the
    pack's bf16 `w` is the optimizer's shadow and the pack's bias IS the master's bias slice, so the forward pass behind a step
    runs on the new weights with no copy.  The model owns the trainer (Module.to): a later to() writes the masters back into
    net.heads (the per-head ConvModules, the source of truth), fuses, repacks, and binds the trainer to the new packs with moments and
    powers kept.
    The reference multiplies the loss by loss_scale_value 1024 and divides the gradients by it again; the gradients here are fp32 and no
    scale is applied (grad_scale 1).  optimizer_cfg: train_cfg["optimizer"] (keys of CENTERNET_OPTIMIZER; `type` must be "Adam";
    the global-norm clip is not built across two ranges)."""
    DEFAULTS, REFUSES = CENTERNET_OPTIMIZER, ("max_norm",)

    def _attach(self, net):
        self.net = net
        return net

    def ranges(self):
        return {name: [(getattr(self.net, name).packed, "w", "b")] for name in ("head1", "head2")}

    def blocks(self):
        """(row0, rows, col0, cols) of hm / wh / reg in head2: the live part of the block-diagonal layer"""
        out, row, hc = [], 0, self.net.head_conv
        for k, name in enumerate(("hm", "wh", "reg")):
            c2 = self.net.heads[name][1]
            out.append((row, c2.cout, k * hc, hc))
            row += c2.cout
        return out

    def train_step(self, inp, example, lr, beta1=0.9):
        """One step on a batch: inp = the network input of CenterNet.train_example, example = its target dict -> the dict of
        CenterNet.loss(grad=True) (the loss BEFORE the update) plus `x` (the neck's output), `h` (head1's) and `dh`.  Nothing is read
        back."""
        net, o1, o2 = self.net, self.opts["head1"], self.opts["head2"]
        x = net.backbone(inp)[-1]
        for m in net.neck:
            x = m(x)
        h = net.head1(x)
        head = net.head2(h)
        out = net.loss_op()(head, example, grad=True)
        g, pc1, pc2 = out["grad"], net.head1.packed, net.head2.packed
        det_ops.conv_bwd_weight(h, g, pc2, cout=net.n_out, blocks=self.blocks(), out=(o2.view("w", "grad"), o2.view("b", "grad")))
        dh = det_ops.conv1x1_bwd_data(g, pc2, cout=net.n_out, act=h)
        det_ops.conv_bwd_weight(x, dh, pc1, out=(o1.view("w", "grad"), o1.view("b", "grad")))
        o2.step(lr, beta1)
        o1.step(lr, beta1)
        return dict(out, head=head, x=x, h=h, dh=dh)

    def sync_modules(self):
        """the fp32 masters back into net.heads[name] = (3x3 ConvModule, 1x1 ConvModule) (weight [cout,cin,k,k], bias [cout]), where
        fuse_heads(), weights.py and a repack read them.  A host copy: for export, not for the step."""
        net = self.net
        w1, b1 = self._host(self.opts["head1"], "w", "b", net.head1.packed)
        w2, b2 = self._host(self.opts["head2"], "w", "b", net.head2.packed)
        for (row0, rows, col0, cols), name in zip(self.blocks(), ("hm", "wh", "reg")):
            c1, c2 = net.heads[name]
            c1.weight = w1[col0:col0 + cols, :c1.cin].clone().contiguous()
            c1.bias = b1[col0:col0 + cols].clone()
            c2.weight = w2[row0:row0 + rows, col0:col0 + cols].reshape(rows, cols, 1, 1).clone()
            c2.bias = b2[row0:row0 + rows].clone()


CENTERPOINT_OPTIMIZER = dict(type="Adam", beta2=0.999, eps=1e-8, weight_decay=0.01, max_norm=35.0, grad_scale=1.0)


def identity_bn(bn):
    """A frozen eval-mode BatchNorm (gamma, beta, mean, var, eps) re-expressed so that nn_ops._fold_bn leaves the conv in front of it
    as it is: mean, var and eps stay, gamma = sqrt(var + eps) in the fold's own fp32 expression (its scale is then exactly 1.0) and
    beta = mean (its shift exactly 0).  What a trainer writes back beside a master that already holds the folded weights."""
    _, _, mean, var, eps = bn
    return torch.sqrt(torch.as_tensor(var).to(torch.float32) + eps), mean, mean, var, eps


class CenterPointHeadTrainer(_HeadTrainerBase):
    """Trains every SepHead branch of graphs.CenterHead (the merged first 3x3 convs + ReLU and the grouped last 3x3 convs) on the device
    with the neck and the shared conv frozen: shared conv -> merged first conv (`mid`) -> md_conv2d_grouped (`head`) -> md_cp_loss_grad
    -> md_conv2d_grouped_bwd_weight (mid, g) -> md_conv2d_grouped_bwd_data (g through mid's ReLU: `dmid`) -> md_conv_bwd_weight (shared,
    dmid) in chunks of at most FIRST_CHUNK output channels, each writing its rows of the flat gradient -> md_grad_sumsq -> md_adam_step.
    ONE Adam over ONE flat range [w_first | w_second | b_first | b_second], so the reference's global-norm clip (max_norm 35) covers both
    packs; its shadow is one bf16 buffer the two packs' `w` are views of, and the packs' biases ARE the master's slices, so the forward
    pass behind a step runs on the new weights with no copy.  The first convs' BatchNorm is frozen: the trained parameters are the folded
    pack (weight x scale, shift), the statistics never move (the reference trains with batch statistics; not built).  The head owns the
    trainer (Module.to): a later to() writes the masters back into the per-branch ConvModules (sync_modules), repacks, and binds
    the trainer to the new packs with masters, moments and powers kept.
    optimizer_cfg: train_cfg["optimizer"] (keys of CENTERPOINT_OPTIMIZER; `type` must be "Adam")."""
    DEFAULTS = CENTERPOINT_OPTIMIZER
    FIRST_CHUNK = 256       # MD_CONV_BWD_MAX_COUT

    def _attach(self, head):
        self.head = head
        return head

    def ranges(self):
        return dict(head=[(self.head._first, "w1", "b1"), (self.head._second, "w2", "b2")])

    def train_step(self, feat, example, lr, beta1=0.9):
        """One step on a batch: feat [B,H,W,in_channels] bf16 = the neck's output, example = the dict of det_ops.cp_assign_targets ->
        the dict of CenterHead.loss(grad=True) (the loss BEFORE the update) plus `head`, `shared`, `mid` and `dmid`.  Nothing is read
        back."""
        head, opt = self.head, self.opt
        pc1, pk2 = head._first, head._second
        head_t, sh, mid = head.forward_mid(feat)
        out = head.loss(example, head_t, grad=True)
        g = out["grad"]
        det_ops.conv2d_grouped_bwd_weight(mid, g, pk2, out=(opt.view("w2", "grad"), opt.view("b2", "grad")))
        dmid = det_ops.conv2d_grouped_bwd_data(g, pk2, act=mid)
        gw, gb = opt.view("w1", "grad"), opt.view("b1", "grad")
        rows = gw.shape[0]
        for r0 in range(0, pc1.cout, self.FIRST_CHUNK):
            n = min(self.FIRST_CHUNK, pc1.cout - r0)
            r1 = rows if r0 + n == pc1.cout else r0 + n       # the last chunk writes the pack's padding rows (+0.0) as well
            det_ops.conv_bwd_weight(sh, dmid, pc1, dy_c_off=r0, cout=n, out=(gw[r0:r1], gb[r0:r1]))
        opt.step(lr, beta1)
        return dict(out, head=head_t, shared=sh, mid=mid, dmid=dmid)

    def sync_modules(self):
        """the fp32 masters back into head.tasks[t][name] = (c1, c2) (weight [cout,64,3,3], bias [cout]), where weights.py and a repack
        read them; c1's BatchNorm becomes identity_bn of its frozen statistics, so nn_ops._fold_bn returns the master bit for bit.  A
        host copy: for export, not for the step."""
        pk2 = self.head._second
        w1, b1 = self._host(self.opt, "w1", "b1", self.head._first)
        w2, b2 = self._host(self.opt, "w2", "b2")
        k = pk2.k
        for i, (_, _, c1, c2) in enumerate(self.head.branches()):
            c1.weight = w1[64 * i:64 * i + 64, :c1.cin].clone().contiguous()
            c1.bias = b1[64 * i:64 * i + 64].clone()
            c1.bn = identity_bn(c1.bn)
            r0, c = pk2.w_rows[i], pk2.couts[i]
            c2.weight = w2[r0:r0 + c].reshape(c, k, k, 64).permute(0, 3, 1, 2).clone().contiguous()
            c2.bias = b2[r0:r0 + c].clone()
