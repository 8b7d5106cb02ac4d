"""Inference graphs as sequences of libminddet_hip.so calls (NHWC bf16 activations).

Reference-present graphs (cited per class) and the build-authored two-stage graph (absent from the
reference, SURVEY 0.2 -- standard public architecture, "parity unpinned").  Each module keeps its
fp32 parameters in the reference's layout (`.weight [Cout,Cin,kh,kw]`, `.bn = (gamma, beta, mean,
var, eps)`) so that the CPU oracle (oracle/nets.py) can run the same graph, and a packed bf16 copy
for the kernels.  Random init follows SURVEY 8(d): He-normal std = sqrt(2/(k*k*Cout))
(centernet/src/resnet.py:210-213), BN gamma=1, beta=0, mean~N(0,0.1), var~U(0.5,1.5).
"""
import math
import os

import numpy as np
import torch

from . import det_ops, nn_ops
from .registry import BACKBONES, DETECTORS, HEADS, NECKS, READERS, ROI_HEAD, build_backbone, build_head, build_neck, build_roi_head


# per-level proposal selection (slice, top-k, decode) on a side HIP stream behind the level's conv, joined before the NMS: +0.4 % on
# the benchmark (same-box 1 856 -> 1 863 images/s); 0 = everything on one stream (A/B)
RPN_OVERLAP = os.environ.get("MD_RPN_OVERLAP", "1") == "1"
# stride-1 bottleneck blocks with 64 mid channels (ResNet-50 / 101 stage 1) as ONE md_bottleneck launch instead of three md_conv2d
# launches (bit-identical results; MD_FUSE_BLOCKS=0 keeps the layer-by-layer path for A/B)
FUSE_BLOCKS = os.environ.get("MD_FUSE_BLOCKS", "1") == "1"
# first block of the later stages: conv3 + the strided 1x1 downsample conv as one K-concatenated GEMM (md_conv1x1_dual; MD_FUSE_DUAL=0: two launches)
FUSE_DUAL = os.environ.get("MD_FUSE_DUAL", "1") == "1"
# identity-block boundaries of ResNet stage 2 (128 mid / 512 block channels): conv3 + residual of block b and conv1 of block b + 1 as ONE
# md_pw_chain launch -- the 512-channel tensor is written once and not read back (bit-identical; MD_PW_CHAIN=0: two md_conv2d launches)
PW_CHAIN = os.environ.get("MD_PW_CHAIN", "1") == "1"
RPN_FUSED_HEAD = os.environ.get("MD_RPN_FUSED", "1") == "1"  # 0: two md_conv2d launches per level (A/B)


class SplitForward:
    """`model.forward` on the S equal parts of a batch, each part on its own HIP stream, outputs concatenated in input order.

    Why: a layer's launch ends with a partly filled round of workgroups (Mask R-CNN's 32-image shard: 525 ping-pong tiles on 256 CUs = 2.05
    rounds -> 3) and with completion skew; with two streams the other half's next launch fills those CUs.  Same kernels on the same images
    -> bit-identical outputs (tests/test_split_forward_gpu.py).  Measured r03, same box, tools/two_stream_halves.py: Mask R-CNN R101 b32
    26.50 -> 25.04 ms/step (-5.5 %), YOLOv8l b32 7.50 -> 7.28 (-2.9 %), Faster R-CNN R50 b120 56.74 -> 56.10 (-1.1 %); YOLOv5s b32 gets 60 %
    SLOWER (its 1.8 ms step is host-enqueue-bound: twice the launches); 3 / 4 / 8 streams lose everywhere.  Opt-in per config: test_cfg.streams.
    The lazily built constants of the graph (anchors, segment offsets) are created by one single-stream pass per part shape before two
    streams read them."""

    def __init__(self, model, streams=2):
        self.model, self.n = model, int(streams)
        self._streams = None
        self._primed = set()

    def __call__(self, images, prepare=None, **kw):
        """images: the batch -- or, with `prepare`, a tuple of batch-first tensors that `prepare(*part)` turns into a part's input batch ON the
        part's stream (pre-processing from uint8: otherwise that launch would sit alone on the caller's stream between two joins)"""
        ins = images if isinstance(images, (tuple, list)) else (images,)
        B = ins[0].shape[0]
        if self.n <= 1 or B < self.n or B % self.n or kw.get("return_aux"):
            return self.model.forward(images if prepare is None else prepare(*ins), **kw)
        dev = ins[0].device
        if self._streams is None or self._streams[0].device != dev:   # (a model moved to another GPU gets streams, and a priming pass, there)
            self._streams = [torch.cuda.Stream(device=dev) for _ in range(self.n)]
            self._primed = set()
        step = B // self.n

        def part(i):
            p = [t[i * step:(i + 1) * step] for t in ins]
            return p[0] if prepare is None else prepare(*p)

        cur = torch.cuda.current_stream(dev)
        # the pack generation is part of the key: any .to() (after a weight reload, of the model or of one of its parts) makes new packs and
        # empties the device constants, and the pass that builds those again must be a single-stream one (r03 ADVICE: part 1 would read
        # them unsynchronised)
        key = (Module.generation, step, prepare is not None) + tuple(ins[0].shape[1:])
        if key not in self._primed:
            self.model.forward(part(0), **kw)
            self._primed.add(key)
        outs = []
        for i, st in enumerate(self._streams):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                outs.append(self.model.forward(part(i), **kw))
        for st in self._streams:
            cur.wait_stream(st)
        res = []
        for k in range(len(outs[0])):
            ts = [o[k] for o in outs]
            for t in ts:
                t.record_stream(cur)   # allocated on a part's stream, read (and later freed) on the caller's
            res.append(torch.cat(ts, 0))
        return tuple(res)


def _split_forward_of(model, test_cfg):
    """test_cfg.streams (default 1) -> model.streams and model.forward_split (== model.forward for one stream)"""
    model.streams = int((test_cfg or {}).get("streams", 1))
    model.forward_split = SplitForward(model, model.streams)


class ParamInit:
    """Deterministic parameter source (numpy Generator, seed 7 by default)."""

    def __init__(self, seed=7):
        self.rng = np.random.default_rng(seed)

    def conv(self, cout, cin, k, std=None):
        std = math.sqrt(2.0 / (k * k * cout)) if std is None else std
        return torch.from_numpy(self.rng.normal(0.0, std, (cout, cin, k, k)).astype(np.float32))

    def bn(self, c, eps=1e-5):
        return (torch.ones(c), torch.zeros(c), torch.from_numpy(self.rng.normal(0, 0.1, c).astype(np.float32)),
                torch.from_numpy(self.rng.uniform(0.5, 1.5, c).astype(np.float32)), eps)

    def bias(self, c, value=None, std=0.01):
        if value is not None:
            return torch.full((c,), float(value))
        return torch.from_numpy(self.rng.normal(0, std, c).astype(np.float32))


class Module:
    """Life cycle of everything that holds parameters or sub-modules.  A class names its direct sub-modules in `children()`; a class
    without any is a leaf and packs its own parameters in `_derive`.  `to(device)` is the one place packs are made: it packs the
    children, then `_derive(device)` builds every pack that is derived from theirs (fused blocks, merged convs, stem forms) into plain
    attributes -- so the call that repacks a conv also rebuilds what was made from it -- empties the device constants and advances
    the process-wide pack generation SplitForward keys its priming pass on.
    A module whose packs are trained holds their trainer (an optim head trainer; `_head_trainer` makes, returns and replaces it) as
    `_trainer`, because the trainer's buffers are derived from those packs too: to() first has it write its fp32 masters back into
    the modules (sync_modules(): they are the source of truth of a repack), then lets `_refresh()` rebuild the children's weights
    that derive from other modules, packs the children, `_derive`s, and last binds the trainer to the new packs (bind(): masters,
    moments and powers kept).  A direct `_derive` call binds nothing.
    `_lazy(name, build)` keeps an operator that is built on first use (a loss, an augmentation) on the instance; to() leaves those."""
    generation = 0
    _trainer = None
    TRAIN_CFG_HINT = ""      # where a training config of this class is found: the end of _train_cfg's message

    def children(self):
        return []

    def modules(self):
        """the leaves under this module, in children order"""
        ch = self.children()
        return [m for c in ch for m in c.modules()] if ch else [self]

    conv_modules = modules

    def to(self, device):
        if self._trainer is not None:
            self._trainer.sync_modules()
        self._refresh()
        for c in self.children():
            c.to(device)
        self._derive(device)
        if self._trainer is not None:
            self._trainer.bind()
        self._consts = {}
        Module.generation += 1
        return self

    def _refresh(self):
        pass

    def _derive(self, device):
        pass

    def const(self, key, build):
        """a shape-dependent device constant (anchors, segment tables, a side stream): built on first use, dropped by to()"""
        if key not in self._consts:
            self._consts[key] = build()
        return self._consts[key]

    def _lazy(self, name, build):
        ops = self.__dict__.setdefault("_ops", {})
        if name not in ops:
            ops[name] = build()
        return ops[name]

    def _train_cfg(self, key):
        if not self.train_cfg or key not in self.train_cfg:
            raise ValueError(f"{type(self).__name__}: train_cfg[{key!r}] is needed for training (see {self.TRAIN_CFG_HINT})")
        return self.train_cfg[key]

    def _head_trainer(self, cls, model, optimizer_cfg, fallback, rederive):
        """The one trainer of this module's packs, cls(model, config): without an optimizer_cfg the existing one, or the first, made
        with `fallback`; with one a new trainer (fresh moments) in place of the existing one, which first leaves its masters in the
        modules and lets go of the packs (it keeps its own buffers and step count), `rederive()` then rebuilding this module's packs
        from the modules on their device."""
        if optimizer_cfg is None and self._trainer is not None:
            return self._trainer
        if self._trainer is not None:
            self._trainer.sync_modules()
            self._trainer = None
            rederive()
        return cls(model, optimizer_cfg if optimizer_cfg is not None else fallback)


def _segments(B, n, device):
    """[0, n, 2 n, ..., B n] int32: the segment table of B equal segments (det_ops.topk_segmented)"""
    return torch.arange(0, (B + 1) * n, n, dtype=torch.int32, device=device)


def _image_hw(images):
    """(H, W) of the images in a batch; in the stem layout (nn_ops.to_stem_layout) the border is not image"""
    border = nn_ops.STEM_PAD_LO + nn_ops.STEM_PAD_HI if images.shape[3] == 4 else 0
    return images.shape[1] - border, images.shape[2] - border


class ConvModule(Module):
    """Conv2d [+ BatchNorm2d(eval)] [+ ReLU] -> one md_conv2d call."""

    def __init__(self, init, cin, cout, k, stride=1, pad=0, bn=True, relu=True, bias=False, bn_eps=1e-5, std=None,
                 bias_value=None, act=None):
        # act: None -> `relu` decides ('relu' after the residual add / none); 'silu' -> SiLU before the residual add
        self.act = act if act is not None else ("relu" if relu else None)
        relu = self.act == "relu"
        self.cin, self.cout, self.k, self.stride, self.pad, self.relu = cin, cout, k, stride, pad, relu
        self.weight = init.conv(cout, cin, k, std)
        self.bn = init.bn(cout, bn_eps) if bn else None
        self.bias = init.bias(cout, bias_value) if bias else None
        self.packed = None

    def _derive(self, device):
        self.packed = nn_ops.pack_conv(self.weight, bias=self.bias, bn=self.bn, stride=self.stride, pad=self.pad,
                                       relu=self.act).to(device)

    def __call__(self, x, residual=None, out=None, c_off=0, x_c_off=None, res_c_off=None):
        return nn_ops.conv2d(x, self.packed, residual=residual, out=out, c_off=c_off, x_c_off=x_c_off, res_c_off=res_c_off)

    def macs(self, ho, wo):
        return ho * wo * self.cout * self.cin * self.k * self.k


def merged_conv(mods, device):
    """Several ConvModules that read the same input (same kernel / stride / pad / activation) as ONE md_conv2d launch whose
    output channels are the modules' outputs side by side: the same arithmetic per output channel, the input read once."""
    m0 = mods[0]
    if any((m.cin, m.k, m.stride, m.pad, m.act, m.bn is None, m.bias is None) != (m0.cin, m0.k, m0.stride, m0.pad, m0.act, m0.bn is None, m0.bias is None)
           for m in mods):
        raise ValueError("merged_conv: the convs must share input, geometry and activation")
    w = torch.cat([m.weight for m in mods], 0)
    bn = None if m0.bn is None else tuple(torch.cat([torch.as_tensor(m.bn[i]) for m in mods]) for i in range(4)) + (m0.bn[4],)
    bias = None if m0.bias is None else torch.cat([m.bias for m in mods])
    return nn_ops.pack_conv(w, bias=bias, bn=bn, stride=m0.stride, pad=m0.pad, relu=m0.act).to(device)


# ----------------------------------------------------------------------------- ResNet (centernet/src/resnet.py)
class BasicBlock(Module):
    """centernet/src/resnet.py:109-136"""
    expansion = 1

    def __init__(self, init, inplanes, planes, stride=1, downsample=None):
        self.conv1 = ConvModule(init, inplanes, planes, 3, stride, 1)
        self.conv2 = ConvModule(init, planes, planes, 3, 1, 1, relu=True)  # ReLU applied after the residual add
        self.downsample = downsample

    def children(self):
        return [self.conv1, self.conv2] + ([self.downsample] if self.downsample else [])

    def __call__(self, x):
        residual = self.downsample(x) if self.downsample is not None else x
        out = self.conv1(x)
        return self.conv2(out, residual=residual)


class Bottleneck(Module):
    """centernet/src/resnet.py:139-178 (stride on the 3x3 conv)"""
    expansion = 4

    def __init__(self, init, inplanes, planes, stride=1, downsample=None):
        self.conv1 = ConvModule(init, inplanes, planes, 1)
        self.conv2 = ConvModule(init, planes, planes, 3, stride, 1)
        self.conv3 = ConvModule(init, planes, planes * 4, 1, relu=True)  # ReLU after the residual add
        self.downsample = downsample
        self._fused = self._dual = None   # the md_bottleneck / md_conv1x1_dual packs (None: the kernel does not take this block)

    def children(self):
        return [self.conv1, self.conv2, self.conv3] + ([self.downsample] if self.downsample else [])

    def _derive(self, device):
        # (PackedDual and PackedBottleneck.b12 hold their own copies of the conv packs' numbers)
        pd = self.downsample.packed if self.downsample is not None else None
        self._fused = nn_ops.pack_bottleneck(self.conv1.packed, self.conv2.packed, self.conv3.packed, pd)
        self._dual = nn_ops.pack_dual(self.conv3.packed, pd) if pd is not None else None

    def __call__(self, x, t1=None, chain=None):
        """t1: conv1(x), where the block in front has computed it in its tail; chain: the md_pw_chain pack of (this conv3, the next block's
        conv1) -- the call then returns (y, the next block's t1).  Both are for identity blocks on the layer-by-layer path only."""
        if t1 is None and chain is None:
            if FUSE_BLOCKS and self._fused is not None:
                # one launch for the whole block (md_bottleneck): x is read once, the 64-channel intermediates stay in LDS, and the
                # first block's 1x1 downsample conv is computed from the same x tile
                res = self.downsample(x) if (self.downsample is not None and self._fused.wd is None) else None
                return nn_ops.bottleneck(x, self._fused, residual=res)
            if FUSE_DUAL and self._dual is not None:
                # first block of a stage: conv3 and the (strided) 1x1 downsample conv as ONE GEMM over [t2 ; x] (md_conv1x1_dual)
                return nn_ops.conv1x1_dual(self.conv2(self.conv1(x)), x, self._dual)
        residual = self.downsample(x) if self.downsample is not None else x
        t2 = self.conv2(self.conv1(x) if t1 is None else t1)
        if chain is not None:
            return nn_ops.pw_chain(t2, residual, chain)
        return self.conv3(t2, residual=residual)


@BACKBONES.register_module
class ResNet(Module):
    """centernet/src/resnet.py:181-252: 7x7/2 stem + BN + ReLU, zero-pad + MaxPool(3,2), 4 stages;
    returns (C2, C3, C4, C5).  depth 18/34 -> BasicBlock, 50/101 -> Bottleneck."""
    SETTINGS = {18: (BasicBlock, [2, 2, 2, 2]), 34: (BasicBlock, [3, 4, 6, 3]), 50: (Bottleneck, [3, 4, 6, 3]),
                101: (Bottleneck, [3, 4, 23, 3])}

    def __init__(self, depth=50, base_width=64, seed=7, init=None, layers=None):
        block, default_layers = self.SETTINGS[depth]
        layers = layers or default_layers
        init = init or ParamInit(seed)
        self.block, self.inplanes = block, base_width
        self.conv1 = ConvModule(init, 3, base_width, 7, 2, 3)
        self.stages = []
        for i, n in enumerate(layers):
            self.stages.append(self._make_layer(init, block, base_width * (2 ** i), n, 1 if i == 0 else 2))
        self.out_channels = [base_width * (2 ** i) * block.expansion for i in range(4)]

    def _make_layer(self, init, block, planes, blocks, stride):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = ConvModule(init, self.inplanes, planes * block.expansion, 1, stride, 0, relu=False)
        layers = [block(init, self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(init, self.inplanes, planes))
        return layers

    def children(self):
        return [self.conv1] + [b for st in self.stages for b in st]

    def _derive(self, device):
        self.stem = None
        if self.conv1.cout == 64 and self.conv1.relu:  # the fused conv + BN + ReLU + maxpool kernel (md_stem_pool)
            self.stem = nn_ops.pack_stem(self.conv1.weight, bn=self.conv1.bn, bias=self.conv1.bias).to(device)
        # md_pw_chain packs, keyed by (stage, block): the tail of identity block b with the head of block b + 1 (they hold the blocks'
        # own pack tensors, so ResNet.to() is the call that makes them)
        self._chains = {}
        if self.block is Bottleneck:
            for si, st in enumerate(self.stages):
                for bi in range(1, len(st) - 1):
                    if st[bi].downsample is None and st[bi + 1].downsample is None and st[bi]._fused is None and st[bi + 1]._fused is None:
                        pk = nn_ops.pack_pw_chain(st[bi].conv3.packed, st[bi + 1].conv1.packed)
                        if pk is not None:
                            self._chains[(si, bi)] = pk

    def __call__(self, x):
        """x: [N,H,W,8] bf16 NHWC (3 real channels), or the same batch already in the stem layout
        ([N,H+16,W+16,4], nn_ops.to_stem_layout) -- then the whole stem is one launch."""
        if x.shape[3] == 4:
            if self.stem is None:
                raise nn_ops._lib.MindDetHipError("ResNet: stem-layout input needs the 64-channel ReLU stem")
            x = nn_ops.stem_pool(x, self.stem)
        else:
            x = self.conv1(x)
            x = nn_ops.maxpool2d(x, 3, 2, 1, zero_pad=True)
        outs = []
        for si, st in enumerate(self.stages):
            t1 = None
            for bi, b in enumerate(st):
                chain = self._chains.get((si, bi)) if PW_CHAIN else None
                if chain is not None:
                    x, t1 = b(x, t1=t1, chain=chain)      # ... and conv1 of block bi + 1
                elif t1 is not None:
                    x, t1 = b(x, t1=t1), None
                else:
                    x = b(x)
            outs.append(x)
        return tuple(outs)


# ----------------------------------------------------------------------------- FPN / RPN / RoI head (build-authored)
@NECKS.register_module
class FPN(Module):
    """Lin et al. 2017: 1x1 laterals, top-down nearest upsample + add, 3x3 output convs, extra level by
    stride-2 subsampling (max_pool k=1 s=2) of the last output.  parity unpinned."""

    def __init__(self, in_channels, out_channels=256, num_outs=5, seed=11, init=None):
        init = init or ParamInit(seed)
        self.lateral = [ConvModule(init, c, out_channels, 1, bn=False, relu=False, bias=True) for c in in_channels]
        self.output = [ConvModule(init, out_channels, out_channels, 3, 1, 1, bn=False, relu=False, bias=True)
                       for _ in in_channels]
        self.num_outs = num_outs

    def children(self):
        return self.lateral + self.output

    def __call__(self, feats):
        # top-down path: lateral_i + nearest_up(merged_{i+1}).  When the pyramid halves exactly the add is fused into
        # the lateral 1x1 conv as an upsampled residual (md_conv2d res_upsample); otherwise the streaming kernel runs.
        lats = [None] * len(feats)
        lats[-1] = self.lateral[-1](feats[-1])
        for i in range(len(feats) - 2, -1, -1):
            h, w = feats[i].shape[1], feats[i].shape[2]
            top = lats[i + 1]
            if top.shape[1] == (h + 1) // 2 and top.shape[2] == (w + 1) // 2:
                lats[i] = nn_ops.conv2d(feats[i], self.lateral[i].packed, residual=top, res_upsample=True)
            else:
                lats[i] = nn_ops.upsample_add(self.lateral[i](feats[i]), top)
        outs = [o(l) for o, l in zip(self.output, lats)]
        while len(outs) < self.num_outs:
            outs.append(nn_ops.maxpool2d(outs[-1], 1, 2, 0, zero_pad=False))
        return outs


@HEADS.register_module
class RPNHead(Module):
    """Shared 3x3 conv + ReLU, then one fused 1x1 conv producing [A objectness | 4A deltas] channels.
    Proposal generation: per level top-k (nms_pre) on the logits, delta2bbox + clip, NMS (iou_thr),
    per image top-`max_per_img` across levels.  parity unpinned (absent from the reference)."""

    def __init__(self, in_channels=256, feat_channels=256, strides=(4, 8, 16, 32, 64), scale=8.0,
                 ratios=(0.5, 1.0, 2.0), nms_pre=1000, max_per_img=1000, nms_thr=0.7, seed=13, init=None):
        init = init or ParamInit(seed)
        self.A = len(ratios)
        self.conv = ConvModule(init, in_channels, feat_channels, 3, 1, 1, bn=False, relu=True, bias=True, std=0.01)
        self.out = ConvModule(init, feat_channels, 5 * self.A, 1, bn=False, relu=False, bias=True, std=0.01)
        self.strides, self.scale, self.ratios = tuple(strides), scale, tuple(ratios)
        self.nms_pre, self.max_per_img, self.nms_thr = nms_pre, max_per_img, nms_thr

    def children(self):
        return [self.conv, self.out]

    def _static(self, feats, img_hw):
        B, dev = feats[0].shape[0], feats[0].device
        sizes = tuple((f.shape[1], f.shape[2]) for f in feats)

        def build():
            anchors = det_ops.fpn_anchors(sizes, self.strides, self.scale, self.ratios, device=dev)
            per, offs, o = [], [], 0
            for (h, w) in sizes:
                n = h * w * self.A
                per.append(anchors[o:o + n])
                offs.append(_segments(B, n, dev))
                o += n
            return dict(anchors=per, seg=offs, merged_seg=_segments(B, len(sizes) * self.nms_pre, dev))

        return self.const((B, sizes, img_hw), build)

    def __call__(self, feats, img_hw):
        st = self._static(feats, img_hw)
        B, L, k, A = feats[0].shape[0], len(feats), self.nms_pre, self.A
        dev = feats[0].device
        boxes = torch.empty((L, B, k, 4), dtype=torch.float32, device=dev)
        scores = torch.empty((L, B, k), dtype=torch.float32, device=dev)
        counts = torch.empty((L, B), dtype=torch.int32, device=dev)
        heads = []
        # RPN_OVERLAP: the per-level selection (slice, top-k, decode: small latency-bound launches) runs on a side stream behind the
        # level's conv while the main stream goes on with the next level's conv; the streams join before the NMS
        main = torch.cuda.current_stream(dev) if RPN_OVERLAP else None
        side = self.const("side", lambda: torch.cuda.Stream(dev)) if RPN_OVERLAP else None
        keep_alive = []
        if RPN_OVERLAP:
            # written on the side stream, allocated on the main one: the caching allocator must not hand their memory to a
            # main-stream allocation while side-stream work may still touch it, whatever happens to the Python references
            for t in (boxes, scores, counts):
                t.record_stream(side)
        try:
            for l, f in enumerate(feats):
                if RPN_FUSED_HEAD and self.conv.cout == 256 and self.out.packed.cout == 16 and self.conv.relu:
                    head = nn_ops.conv2d_head(f, self.conv.packed, self.out.packed)   # [B,H,W,16], one launch per level
                else:
                    head = self.out(self.conv(f))
                heads.append(head)

                def select(l=l, f=f, head=head):
                    logits = nn_ops.slice_cast(head, 0, A)              # [B,H,W,A] fp32
                    _, idx, cnt = det_ops.topk_segmented(logits, st["seg"][l], k, out_cnt=counts[l],
                                                         max_segment=f.shape[1] * f.shape[2] * A)
                    det_ops.rpn_decode(head, st["anchors"][l], idx, cnt, A, img_hw, out_boxes=boxes[l], out_scores=scores[l])
                    keep_alive.append((logits, idx, cnt))

                if RPN_OVERLAP:
                    head.record_stream(side)
                    ev = torch.cuda.Event()
                    ev.record(main)
                    with torch.cuda.stream(side):
                        side.wait_event(ev)
                        select()
                else:
                    select()
        finally:
            if RPN_OVERLAP:
                main.wait_stream(side)   # always joined, also when a level's selection raised
        keep, _, _ = det_ops.nms_aligned(boxes.view(L * B, k, 4), self.nms_thr, mode=det_ops.NMS_MODE_STRICT,
                                         count=counts.view(-1))
        mboxes, mscores = det_ops.rpn_merge(boxes, scores, keep.view(L, B, k))
        topv, topi, cnt = det_ops.topk_segmented(mscores, st["merged_seg"], self.max_per_img, max_segment=L * k)
        rois, roi_scores = det_ops.make_rois(mboxes, topv, topi, cnt)
        return rois, roi_scores, cnt, dict(heads=heads, boxes=boxes, scores=scores, counts=counts, keep=keep,
                                           mboxes=mboxes, mscores=mscores)


@ROI_HEAD.register_module
class StandardRoIHead(Module):
    """RoIAlign 7x7 over P2..P5 -> FC 1024 -> FC 1024 -> fused [cls (nc+1) | reg (4 nc)] FC, softmax,
    class-specific delta2bbox, score threshold, class-wise NMS, top max_per_img.  parity unpinned."""

    def __init__(self, in_channels=256, fc_channels=1024, num_classes=80, roi_size=7, sampling_ratio=2,
                 featmap_strides=(4, 8, 16, 32), score_thr=0.05, nms_thr=0.5, max_per_img=100, nms_pre=2048,
                 seed=17, init=None):
        init = init or ParamInit(seed)
        self.nc, self.P, self.C = num_classes, roi_size, in_channels
        k_in = in_channels * roi_size * roi_size
        # FC weights are stored in the conv layout [Cout, Cin, 1, 1]; fc1's Cin axis is ordered (h, w, c) to
        # match the NHWC RoIAlign output flattened as-is.
        self.fc1 = ConvModule(init, k_in, fc_channels, 1, bn=False, relu=True, bias=True, std=math.sqrt(2.0 / k_in))
        self.fc2 = ConvModule(init, fc_channels, fc_channels, 1, bn=False, relu=True, bias=True,
                              std=math.sqrt(2.0 / fc_channels))
        self.reg_offset = (num_classes + 1 + 7) // 8 * 8
        n_out = self.reg_offset + 4 * num_classes
        self.fc_out = ConvModule(init, fc_channels, n_out, 1, bn=False, relu=False, bias=True, std=0.01)
        # channels [nc+1, reg_offset) are alignment padding: zero their weights so they stay inert
        self.fc_out.weight[num_classes + 1:self.reg_offset] = 0
        self.fc_out.bias[num_classes + 1:self.reg_offset] = 0
        # class logits get a wider init so that the synthetic benchmark has above-threshold candidates
        self.fc_out.weight[:num_classes + 1] *= 20.0
        self.strides, self.sampling = tuple(featmap_strides), sampling_ratio
        self.score_thr, self.nms_thr, self.max_per_img, self.nms_pre = score_thr, nms_thr, max_per_img, nms_pre
        # nms_pre: the class-wise NMS runs on the top-nms_pre (roi, class) candidates of an image instead of on all of them (the
        # public definition: every candidate above score_thr).  The cut is result-identical whenever the prefix yields max_per_img
        # survivors or was not full; the one other case raises a sticky per-image flag on the device (DESIGN.md "pre-NMS prefix")
        self.prefix_status = det_ops.PrefixStatus()

    def children(self):
        return [self.fc1, self.fc2, self.fc_out]

    def __call__(self, feats, rois, roi_cnt, img_hw):
        B = feats[0].shape[0]
        R = rois.shape[0]
        post = R // B
        dev = rois.device
        pooled = det_ops.roi_align(list(feats[:len(self.strides)]), rois, self.P, [1.0 / s for s in self.strides],
                                   self.sampling, True)
        x = nn_ops.linear(pooled.view(R, self.P * self.P * self.C), self.fc1.packed)
        x = nn_ops.linear(x, self.fc2.packed)
        cls_reg = nn_ops.linear(x, self.fc_out.packed)
        cand = det_ops.rcnn_scores(cls_reg, roi_cnt, self.nc, self.score_thr)
        seg = self.const((B, post), lambda: _segments(B, post * self.nc, dev))
        sv, si, sc = det_ops.topk_segmented(cand, seg, self.nms_pre, max_segment=post * self.nc)
        boxes, labels = det_ops.rcnn_decode_selected(cls_reg, rois, si, sc, self.nc, self.reg_offset, img_hw)
        keep, kidx, num = det_ops.nms_aligned(boxes, self.nms_thr, mode=det_ops.NMS_MODE_STRICT, count=sc, group=labels,
                                              max_output=self.max_per_img)
        dets, count = det_ops.pack_detections(boxes, sv, labels, kidx, num, self.max_per_img, sel_cnt=sc,
                                              status=self.prefix_status.tensor(B, dev))
        return dets, count, dict(pooled=pooled, cls_reg=cls_reg, cand=cand, sel_scores=sv, sel_idx=si, sel_cnt=sc,
                                 boxes=boxes, labels=labels, keep=keep)


@DETECTORS.register_module
class FasterRCNN(Module):
    """Two-stage detector: backbone -> neck -> rpn_head -> roi_head.  `forward(images)` takes
    [B,H,W,8] bf16 NHWC (RGB in channels 0..2, 5 zero channels) and returns (dets [B,max_det,6], count [B])."""

    def __init__(self, backbone, neck, rpn_head, roi_head, train_cfg=None, test_cfg=None):
        self.backbone = build_backbone(backbone)
        neck = dict(neck)
        neck.setdefault("in_channels", self.backbone.out_channels)
        self.neck = build_neck(neck)
        self.rpn_head = build_head(rpn_head)
        self.roi_head = build_roi_head(roi_head)
        self.test_cfg = test_cfg
        _split_forward_of(self, test_cfg)

    def children(self):
        return [self.backbone, self.neck, self.rpn_head, self.roi_head]

    @property
    def prefix_status(self):
        """sticky device flags of the second stage's top-nms_pre cut (det_ops.PrefixStatus)"""
        return self.roi_head.prefix_status

    def extract_feat(self, images):
        return self.neck(self.backbone(images))

    def forward(self, images, return_aux=False):
        img_hw = _image_hw(images)
        feats = self.extract_feat(images)
        rois, roi_scores, roi_cnt, aux_rpn = self.rpn_head(feats, img_hw)
        dets, count, aux_roi = self.roi_head(feats, rois, roi_cnt, img_hw)
        if return_aux:
            return dets, count, dict(feats=feats, rois=rois, roi_scores=roi_scores, roi_cnt=roi_cnt, rpn=aux_rpn, roi=aux_roi)
        return dets, count

    __call__ = forward

    def macs_per_image(self, h, w, num_rois=None):
        """Algorithmic MACs (SURVEY 8d formula) of every conv/FC for one h x w image."""
        total, hh, ww = 0, h, w
        bb = self.backbone

        def out_hw(m, hh, ww):
            return (hh + 2 * m.pad - m.k) // m.stride + 1, (ww + 2 * m.pad - m.k) // m.stride + 1

        hh, ww = out_hw(bb.conv1, hh, ww)
        total += bb.conv1.macs(hh, ww)
        hh, ww = (hh + 2 - 3) // 2 + 1, (ww + 2 - 3) // 2 + 1
        sizes = []
        for st in bb.stages:
            for b in st:
                h_in, w_in = hh, ww
                for m in b.modules():
                    if m is b.downsample:
                        ho, wo = out_hw(m, h_in, w_in)
                        total += m.macs(ho, wo)
                    else:
                        hh, ww = out_hw(m, hh, ww)
                        total += m.macs(hh, ww)
            sizes.append((hh, ww))
        for l, (a, b_) in zip(self.neck.lateral, sizes):
            total += l.macs(a, b_)
        for o, (a, b_) in zip(self.neck.output, sizes):
            total += o.macs(a, b_)
        lv = list(sizes)
        while len(lv) < self.neck.num_outs:
            lv.append(((lv[-1][0] - 1) // 2 + 1, (lv[-1][1] - 1) // 2 + 1))
        for (a, b_) in lv:
            total += self.rpn_head.conv.macs(a, b_) + self.rpn_head.out.macs(a, b_)
        r = num_rois if num_rois is not None else self.rpn_head.max_per_img
        for m in self.roi_head.modules():
            total += r * m.cout * m.cin
        return total


# ----------------------------------------------------------------------------- CenterNet (reference-present graph)
class DeconvModule(Module):
    """Conv2dTranspose [+ BatchNorm2d] [+ ReLU] -> s*s sub-pixel md_conv2d launches (nn_ops.pack_conv_transpose)."""

    def __init__(self, init, cin, cout, k, stride, pad, bn=True, relu=True, bn_eps=1e-5):
        self.cin, self.cout, self.k, self.stride, self.pad, self.relu = cin, cout, k, stride, pad, relu
        std = math.sqrt(2.0 / (k * k * cout))
        self.weight_t = torch.from_numpy(init.rng.normal(0.0, std, (cin, cout, k, k)).astype(np.float32))
        self.bn = init.bn(cout, bn_eps) if bn else None
        self.packed = None

    def _derive(self, device):
        self.packed = nn_ops.pack_conv_transpose(self.weight_t, bn=self.bn, stride=self.stride, pad=self.pad,
                                                 relu=self.relu).to(device)

    def __call__(self, x, out=None, c_off=0):
        return nn_ops.conv_transpose2d(x, self.packed, out=out, c_off=c_off)


@ROI_HEAD.register_module
class FCNMaskHead(Module):
    """Mask R-CNN mask branch (He et al. 2017, FPN variant): RoIAlign 14x14 over P2..P5 on the final detections -> 4 x
    [3x3 conv 256 + ReLU] -> Conv2dTranspose 2x2 s2 + ReLU -> 1x1 conv to num_classes -> the detection's own class channel,
    sigmoid: [B, max_det, 28, 28].  Absent from the reference (Mask R-CNN is a README bullet): parity unpinned."""

    def __init__(self, in_channels=256, conv_channels=256, num_convs=4, num_classes=80, roi_size=14, sampling_ratio=2,
                 featmap_strides=(4, 8, 16, 32), seed=19, init=None):
        init = init or ParamInit(seed)
        self.nc, self.P, self.C = num_classes, roi_size, in_channels
        self.convs = []
        cin = in_channels
        for _ in range(num_convs):
            self.convs.append(ConvModule(init, cin, conv_channels, 3, 1, 1, bn=False, relu=True, bias=True))
            cin = conv_channels
        self.upsample = DeconvModule(init, cin, conv_channels, 2, 2, 0, bn=False, relu=True)
        self.logits = ConvModule(init, conv_channels, num_classes, 1, bn=False, relu=False, bias=True, std=0.05)
        self.strides, self.sampling = tuple(featmap_strides), sampling_ratio

    def children(self):
        return self.convs + [self.upsample, self.logits]

    def __call__(self, feats, dets):
        B, D = dets.shape[0], dets.shape[1]
        rois = det_ops.dets_to_rois(dets)                                          # [B*D, 5]
        x = det_ops.roi_align(list(feats[:len(self.strides)]), rois, self.P, [1.0 / s for s in self.strides], self.sampling, True)
        for m in self.convs:
            x = m(x)
        x = self.logits(self.upsample(x))                                          # [B*D, 2P, 2P, nc (padded to 8)]
        masks = det_ops.mask_select(x, dets.view(B * D, 6), self.nc)
        return masks.view(B, D, 2 * self.P, 2 * self.P), dict(rois=rois, logits=x)


@DETECTORS.register_module
class MaskRCNN(FasterRCNN):
    """Faster R-CNN + FCNMaskHead on the final detections: forward -> (dets [B,max_det,6], count [B], masks [B,max_det,28,28]).
    test_cfg.paste_masks (or forward(paste=True)): a fourth output, the masks pasted into the image at `mask_thr_binary` (md_paste_masks):
    [B,max_det,H,ceil(W/32)] int32 bit masks (bit j of word k of a row = pixel 32 k + j)."""

    def __init__(self, backbone, neck, rpn_head, roi_head, mask_head, train_cfg=None, test_cfg=None):
        super().__init__(backbone, neck, rpn_head, roi_head, train_cfg, test_cfg)
        self.mask_head = build_roi_head(mask_head)
        tc = test_cfg or {}
        self.paste = bool(tc.get("paste_masks", False))
        self.mask_thr = float(tc.get("mask_thr_binary", 0.5))

    def children(self):
        return super().children() + [self.mask_head]

    def forward(self, images, return_aux=False, paste=None):
        dets, count, aux = FasterRCNN.forward(self, images, return_aux=True)
        masks, aux_mask = self.mask_head(aux["feats"], dets)
        out = (dets, count, masks)
        if self.paste if paste is None else paste:
            out = out + (det_ops.paste_masks(masks, dets, _image_hw(images), self.mask_thr, bits=True),)
        if return_aux:
            aux["mask"] = aux_mask
            return out + (aux,)
        return out

    __call__ = forward


class DeformConvModule(Module):
    """ModulatedDeformConv2d (DCNv2) + BatchNorm2d + ReLU -- centernet/src/resnet.py:24-106, used by the CenterNet neck
    (centernet_det.py:123-160): offset conv (3*k*k channels, has_bias) -> md_deform_cols -> 1x1 md_conv2d over the columns.
    The reference zero-initialises the offset conv; here it gets a small random init so that random-weight runs and tests
    exercise the sampling path."""

    def __init__(self, init, cin, cout, k=3, stride=1, pad=1, bn=True, relu=True, bn_eps=1e-5, offset_std=0.02):
        self.cin, self.cout, self.k, self.stride, self.pad, self.relu = cin, cout, k, stride, pad, relu
        self.act = "relu" if relu else None
        self.weight = init.conv(cout, cin, k, None)
        self.bn = init.bn(cout, bn_eps) if bn else None
        self.bias = None
        self.offset_weight = init.conv(3 * k * k, cin, k, offset_std)
        self.offset_bias = torch.from_numpy(init.rng.normal(0.0, 0.1, (3 * k * k,)).astype(np.float32))
        self.packed = self.packed_offset = None

    def _derive(self, device):
        self.packed = nn_ops.pack_conv(self.weight, bias=self.bias, bn=self.bn, stride=self.stride, pad=self.pad, relu=self.act,
                                       korder=0).to(device)
        self.packed_offset = nn_ops.pack_conv(self.offset_weight, bias=self.offset_bias, stride=self.stride, pad=self.pad,
                                              relu=False).to(device)

    def __call__(self, x):
        return nn_ops.deform_conv2d(x, self.packed_offset, self.packed)

    def macs(self, ho, wo):
        return ho * wo * (self.cout + 3 * self.k * self.k) * self.cin * self.k * self.k


@DETECTORS.register_module
class CenterNet(Module):
    """centernet/src/centernet_det.py:79-174 (GatherDetectionFeatureCell) + :374-399 (CenterNetDetEval):
    ResNet-18 -> 3 x [3x3 conv + BN + ReLU, Conv2dTranspose 4x4 s2 p1 + BN + ReLU] (512->256->128->64)
    -> hm / wh / reg heads (3x3 conv 64 + ReLU, 1x1 conv; hm bias -2.19, :29-69) -> sigmoid+clip ->
    DetectionDecode (decode.py:123-196).
    The three ModulatedDeformConv2d 3x3 layers (DCNv2, resnet.py:24-106) run as DeformConvModule (published DCNv2
    definition: the primitive's arithmetic is inside un-vendored MindSpore, parity unpinned); `dcn=False` substitutes plain
    3x3 convs.
    The three heads are evaluated as one fused 3x3 conv (64 -> 3*head_conv) and one block-diagonal 1x1
    conv (same arithmetic per output: the off-block weights are exact zeros)."""

    def __init__(self, depth=18, num_classes=80, head_conv=64, K=100, base_width=64, seed=7, train_cfg=None,
                 test_cfg=None, dcn=True):
        init = ParamInit(seed)
        _split_forward_of(self, test_cfg)
        self.backbone = ResNet(depth, base_width=base_width, init=init)
        cin = self.backbone.out_channels[-1]
        self.neck = []
        for cout in (base_width * 4, base_width * 2, base_width):
            self.neck.append(DeformConvModule(init, cin, cout, 3, 1, 1) if dcn else ConvModule(init, cin, cout, 3, 1, 1))
            self.neck.append(DeconvModule(init, cout, cout, 4, 2, 1))
            cin = cout
        self.num_classes, self.head_conv, self.K = num_classes, head_conv, K
        hc = head_conv
        self.heads = {}
        for name, cout, b2 in (("hm", num_classes, -2.19), ("wh", 2, 0.0), ("reg", 2, 0.0)):
            std = None if name == "hm" else 0.001
            c1 = ConvModule(init, cin, hc, 3, 1, 1, bn=False, relu=True, bias=True, std=std,
                            bias_value=None if name == "hm" else 0.0)
            c2 = ConvModule(init, hc, cout, 1, bn=False, relu=False, bias=True, std=std, bias_value=b2)
            self.heads[name] = (c1, c2)
        # fused forms
        self.head1 = ConvModule(init, cin, 3 * hc, 3, 1, 1, bn=False, relu=True, bias=True)
        self.n_out = num_classes + 4
        self.head2 = ConvModule(init, 3 * hc, self.n_out, 1, bn=False, relu=False, bias=True)
        self.fuse_heads()
        self.decode = det_ops.DetectionDecode(reg_offset=True, K=K)
        self.train_cfg = train_cfg

    def fuse_heads(self):
        """(Re)build the fused head convs' weights from self.heads (to() calls it: they are packed like any other conv)."""
        hc = self.head_conv
        self.head1.weight = torch.cat([self.heads[n][0].weight for n in ("hm", "wh", "reg")], 0)
        self.head1.bias = torch.cat([self.heads[n][0].bias for n in ("hm", "wh", "reg")], 0)
        w2 = torch.zeros((self.n_out, 3 * hc, 1, 1))
        b2 = torch.zeros((self.n_out,))
        o = 0
        for i, n in enumerate(("hm", "wh", "reg")):
            c2 = self.heads[n][1]
            w2[o:o + c2.cout, i * hc:(i + 1) * hc] = c2.weight
            b2[o:o + c2.cout] = c2.bias
            o += c2.cout
        self.head2.weight, self.head2.bias = w2, b2

    def children(self):
        return [self.backbone] + self.neck + [self.head1, self.head2]

    TRAIN_CFG_HINT = "configs/centernet/centernet_r18_dcn_train.py"

    def _refresh(self):
        self.fuse_heads()   # head1 / head2 are children whose weights derive from self.heads (which a trainer has just written)

    def features(self, images):
        x = self.backbone(images)[-1]
        for m in self.neck:
            x = m(x)
        return self.head2(self.head1(x))  # [B, H/4, W/4, roundup8(num_classes + 4)]

    def forward(self, images, return_aux=False):
        head = self.features(images)
        nc = self.num_classes
        # heat map: NHWC bf16 -> NCHW fp32, sigmoid + clip and the 3x3 peak test in one launch (md_heat_peaks)
        heat, hm = det_ops.heat_peaks(head, 0, nc, with_hm=return_aux)
        wh = nn_ops.nhwc_to_nchw_f32(head, nc, 2)
        reg = nn_ops.nhwc_to_nchw_f32(head, nc + 2, 2)
        det, inds, cls = self.decode({"hm": hm, "heat": heat, "wh": wh, "reg": reg}, return_indices=True)
        if return_aux:
            return det, dict(head=head, hm=hm, wh=wh, reg=reg, inds=inds, cls=cls)
        return det

    __call__ = forward

    def loss_op(self):
        """det_ops.CenterNetLoss of this head's layout with the settings of train_cfg (None: the reference's default values)"""
        return self._lazy("loss", lambda: det_ops.CenterNetLoss.from_model(self, self.train_cfg))

    def loss(self, images, example, grad=False):
        """CenterNetLossCell.construct (centernet/src/centernet_det.py:206-237): features(), then the loss on the head tensor.
        example = the dict of det_ops.cn_assign_targets (hm, ind, reg_mask, wh, reg) -> the dict of det_ops.cn_loss (grad=True: with
        d total / d head, the first gradient of a training step) plus `head`, the tensor the gradient belongs to; the differentiable
        form is det_ops.center_net_loss(head, example, self.loss_op())."""
        head = self.features(images)
        return dict(self.loss_op()(head, example, grad=grad), head=head)

    def augment_op(self):
        """det_ops.CenterNetAugment with train_cfg["augment"] on the input of train_cfg["assigner"], in the stem's input layout"""
        def build():
            a = self._train_cfg("assigner")
            return det_ops.CenterNetAugment(a["input_res"], a["down_ratio"], **dict(self._train_cfg("augment")))
        return self._lazy("augment", build)

    def targets_op(self):
        """det_ops.CenterNetTargets with train_cfg["assigner"] for this model's classes"""
        def build():
            a = self._train_cfg("assigner")
            h, w = (int(v) for v in a["input_res"])
            d = int(a["down_ratio"])
            return det_ops.CenterNetTargets(self.num_classes, (w // d, h // d), a["max_objs"], a.get("min_overlap", 0.7))
        return self._lazy("targets", build)

    def train_example(self, images_u8, sizes, bboxes, category_id, generator=None, draws=None, colour=None):
        """Raw images and ground truth -> (input, example) of loss(), on the device with nothing read back: the training branch of
        COCOHP.preprocess_fn (det_ops.CenterNetAugment: images_u8 [B,Hs,Ws,3] uint8 BGR padded to a common extent, sizes [B,2] (h, w);
        draws / colour = the pair of its draw(), None: drawn with `generator`), then the target step (det_ops.CenterNetTargets) on
        bboxes [B,G,4] original-image boxes and category_id [B,G], fed the augmentation's trans_out and flip_width as device tensors.
        -> (the bf16 network input, the dict of det_ops.cn_assign_targets plus trans_out and flip_width)."""
        inp, trans_out, flip_width = self.augment_op()(images_u8, sizes, draws=draws, colour=colour, generator=generator)
        example = self.targets_op()(bboxes, category_id, trans=trans_out, flip_width=flip_width)
        return inp, dict(example, trans_out=trans_out, flip_width=flip_width)

    def train_loss(self, images_u8, sizes, bboxes, category_id, generator=None, draws=None, colour=None, grad=False):
        """train_example, then loss() on the augmented input: raw images + ground truth -> loss (and, grad=True, d total / d head) as
        one device chain.  -> the dict of loss() plus `example`."""
        inp, ex = self.train_example(images_u8, sizes, bboxes, category_id, generator=generator, draws=draws, colour=colour)
        return dict(self.loss(inp, ex, grad=grad), example=ex)

    def head_trainer(self, optimizer_cfg=None):
        """optim.CenterNetHeadTrainer of this model (head1 and head2, the backbone and the neck frozen): train_step(inp, example, lr,
        beta1) continues loss(grad=True) through md_conv_bwd_weight, md_conv1x1_bwd_data and md_adam_step on the device.
        optimizer_cfg: None = train_cfg["optimizer"] (none there: optim.CENTERNET_OPTIMIZER).  One trainer per model: a call without a
        config returns the existing one, a call with one replaces it (fresh moments).  The model has to be on its device."""
        from . import optim

        def rederive():
            device = self.head1.packed.w.device
            self.fuse_heads()
            for m in (self.head1, self.head2):
                m.to(device)
        return self._head_trainer(optim.CenterNetHeadTrainer, self, optimizer_cfg, (self.train_cfg or {}).get("optimizer"), rederive)

    def train_step(self, images_u8, sizes, bboxes, category_id, lr, beta1=0.9, generator=None, draws=None, colour=None):
        """train_example, then one step of head_trainer() on the augmented input: raw images + ground truth -> updated heads as one
        device chain.  -> the dict of CenterNetHeadTrainer.train_step plus `example`."""
        inp, ex = self.train_example(images_u8, sizes, bboxes, category_id, generator=generator, draws=draws, colour=colour)
        return dict(self.head_trainer().train_step(inp, ex, lr, beta1), example=ex)


# ----------------------------------------------------------------------------- CenterPoint RPN neck
@NECKS.register_module
class RPN(Module):
    """centerpoint/det3d_ms/models/necks/rpn.py:9-154: per stage [Pad1 + Conv3x3(stride) + BN(eps 1e-3) + ReLU]
    + n x [Conv3x3 + BN + ReLU]; deblocks = Conv2dTranspose(k=s, stride s) or strided Conv2d(k, stride k)
    + BN + ReLU; channel concat -> [B, H/ds, W/ds, sum(us_num_filters)].  The concat is free: every deblock
    writes its channel slice of the output directly (md_conv2d c_off)."""

    def __init__(self, layer_nums=(3, 5, 5), ds_layer_strides=(2, 2, 2), ds_num_filters=(64, 128, 256),
                 us_layer_strides=(0.5, 1, 2), us_num_filters=(128, 128, 128), num_input_features=64, norm_cfg=None,
                 seed=7, inner_norm_eps=None, **kwargs):
        # inner_norm_eps: per block the BatchNorm eps of the n convs behind the block's first one, None (entry or whole argument) = eps
        init = ParamInit(seed)
        eps = (norm_cfg or {}).get("eps", 1e-3)
        inner = [eps if e is None else float(e) for e in (inner_norm_eps or [None] * len(layer_nums))]
        self.blocks, self.deblocks = [], []
        cin = num_input_features
        self.up_start = len(layer_nums) - len(us_layer_strides)
        for i, n in enumerate(layer_nums):
            blk = [ConvModule(init, cin, ds_num_filters[i], 3, ds_layer_strides[i], 1, bn_eps=eps)]
            blk += [ConvModule(init, ds_num_filters[i], ds_num_filters[i], 3, 1, 1, bn_eps=inner[i]) for _ in range(n)]
            self.blocks.append(blk)
            cin = ds_num_filters[i]
            if i - self.up_start >= 0:
                s = us_layer_strides[i - self.up_start]
                cout = us_num_filters[i - self.up_start]
                if s > 1:
                    self.deblocks.append(DeconvModule(init, cin, cout, int(s), int(s), 0, bn_eps=eps))
                else:
                    k = int(round(1 / s))
                    self.deblocks.append(ConvModule(init, cin, cout, k, k, 0, bn_eps=eps))
        self.out_channels = sum(us_num_filters)

    def children(self):
        return [m for b in self.blocks for m in b] + self.deblocks

    def __call__(self, x):
        out, c_off = None, 0
        for i, blk in enumerate(self.blocks):
            for m in blk:
                x = m(x)
            if i - self.up_start >= 0:
                d = self.deblocks[i - self.up_start]
                if out is None:
                    if isinstance(d, DeconvModule):
                        oh, ow = x.shape[1] * d.stride, x.shape[2] * d.stride
                    else:
                        oh, ow = nn_ops.conv_out_hw(x.shape[1], x.shape[2], d.packed)
                    out = torch.empty((x.shape[0], oh, ow, self.out_channels), dtype=torch.bfloat16, device=x.device)
                if isinstance(d, DeconvModule):
                    d(x, out=out, c_off=c_off)
                else:
                    nn_ops.conv2d(x, d.packed, out=out, c_off=c_off)
                c_off += d.cout
        return out


# ----------------------------------------------------------------------------- CenterPoint head + detector
SEPHEAD_GROUPED = os.environ.get("MD_SEPHEAD_GROUPED", "1") != "0"   # A/B knob: 0 = 36 md_conv2d launches for the SepHead final convs
SEPHEAD_ORDER = ("reg", "height", "dim", "rot", "vel", "hm")         # the dict order of SepHead.construct (center_head.py:85-93)
# post-processing of every task and sample as ONE chain of seven launches (det_ops.CenterHeadPostBatched; bit-identical): MD_CP_POST=1.
# The default stays one CenterHeadPost per task + merge_center_tasks: the production-replay tests pin that pass's operator set
CP_POST = os.environ.get("MD_CP_POST", "0") == "1"


@HEADS.register_module
class CenterHead(Module):
    """centerpoint/det3d_ms/models/bbox_heads/center_head.py:103-200: shared 3x3 conv (in_channels -> share_conv_channel, bias, BN,
    ReLU), then per task a SepHead (:28-99) with one branch per head of common_heads + hm: 3x3 conv 64 -> 64 + bias + BN(eps 1e-5) +
    ReLU, 3x3 conv 64 -> c + bias (hm bias init_bias).  The per-branch ConvModules (self.tasks[t][head] = (c1, c2)) are the source of
    truth; to() rebuilds the fast form from them, three launches: the shared conv, ONE md_conv2d 64 -> 36 x 64 for every branch's
    first conv, ONE md_conv2d_grouped for every branch's last conv into one head tensor [B, H, W, roundup(sum c, 8)] that holds task
    t's heads in SEPHEAD_ORDER from channel task_base[t] (channels past sum c are not written).  MD_SEPHEAD_GROUPED=0 runs the last
    convs as one md_conv2d per branch instead, into [B, H, W, 8 x branches] with branch i at channel 8 i (A/B)."""

    def __init__(self, in_channels=384, tasks=(), common_heads=None, share_conv_channel=64, num_hm_conv=2, init_bias=-2.19, seed=7,
                 dataset="nuscenes", weight=0.25, code_weights=None, logger=None, dcn_head=False):
        if dcn_head:
            raise ValueError("CenterHead: dcn_head is not supported")
        if share_conv_channel != 64 or num_hm_conv != 2:
            raise ValueError("CenterHead: the fast form needs share_conv_channel=64 and two convs per SepHead branch (num_hm_conv=2)")
        common_heads = dict(common_heads or {})
        init = ParamInit(seed)
        self.in_channels, self.share = int(in_channels), int(share_conv_channel)
        self.num_classes = [int(t.get("num_class", len(t["class_names"]))) for t in tasks]
        self.class_names = [list(t["class_names"]) for t in tasks]
        # the loss settings of center_head.py:124-125: the loc-loss weight and one weight per anno_box column (default: all 1)
        self.weight = float(weight)
        self.code_weights = [float(v) for v in code_weights] if code_weights else [1.0] * (10 if "vel" in common_heads else 8)
        self.shared_conv = ConvModule(init, self.in_channels, self.share, 3, 1, 1, bn=True, relu=True, bias=True)
        self.tasks = []
        for nc in self.num_classes:
            heads = dict(common_heads)
            heads["hm"] = (nc, num_hm_conv)
            order = [h for h in SEPHEAD_ORDER if h in heads] + [h for h in heads if h not in SEPHEAD_ORDER]
            sep = {}
            for h in order:
                c = int(heads[h][0])
                if int(heads[h][1]) != 2:
                    raise ValueError(f"CenterHead: head {h!r} has {heads[h][1]} convs; the fast form needs 2")
                c1 = ConvModule(init, self.share, self.share, 3, 1, 1, bn=True, relu=True, bias=True)
                c2 = ConvModule(init, self.share, c, 3, 1, 1, bn=False, relu=False, bias=True,
                                bias_value=init_bias if h == "hm" else None)
                sep[h] = (c1, c2)
            self.tasks.append(sep)
        # channel layout of the head tensor: task t's heads side by side from task_base[t]
        self.offsets, base = [], 0
        for sep in self.tasks:
            off = {}
            for h, (_, c2) in sep.items():
                off[h] = base
                base += c2.cout
            self.offsets.append(off)
        self.head_channels = base
        self.task_base = [min(o.values()) for o in self.offsets]

    def branches(self):
        return [(t, h, c1, c2) for t, sep in enumerate(self.tasks) for h, (c1, c2) in sep.items()]

    def children(self):
        """the convs that are packed alone: the shared conv and every branch's last conv (the A/B path).  The branches' first convs only
        run merged (_derive); branches() lists both."""
        return [self.shared_conv] + [c2 for _, _, _, c2 in self.branches()]

    _first = _second = None     # the merged first convs and the grouped last convs (_derive): what optim.CenterPointHeadTrainer trains

    def _derive(self, device):
        br = self.branches()
        self._first = merged_conv([c1 for _, _, c1, _ in br], device)
        self._second = nn_ops.pack_conv2d_grouped([(c2.weight, c2.bias, None) for _, _, _, c2 in br],
                                                  y_offs=[self.offsets[t][h] for t, h, _, _ in br]).to(device)

    def head_trainer(self, optimizer_cfg=None, fallback=None):
        """optim.CenterPointHeadTrainer of this head (every SepHead branch, first and last convs; the shared conv frozen):
        train_step(feat, example, lr, beta1) continues loss(grad=True) through md_conv2d_grouped_bwd_weight, md_conv2d_grouped_bwd_data,
        md_conv_bwd_weight, md_grad_sumsq and md_adam_step on the device.  optimizer_cfg: None = `fallback`, the config of the
        detector around the head, which has no train_cfg of its own (None: optim.CENTERPOINT_OPTIMIZER).  One trainer per head: a call
        without an optimizer_cfg returns the existing one, a call with one replaces it (fresh moments).  The head has to be on its device."""
        from . import optim

        return self._head_trainer(optim.CenterPointHeadTrainer, self, optimizer_cfg, fallback, lambda: self._derive(self._first.w.device))

    def task_offsets(self, grouped=None):
        """per task {head: first channel} in the head tensor __call__ returns (grouped None: the SEPHEAD_GROUPED setting)"""
        if grouped if grouped is not None else SEPHEAD_GROUPED:
            return [dict(o) for o in self.offsets]
        out, i = [], 0
        for sep in self.tasks:
            out.append({h: 8 * (i + j) for j, h in enumerate(sep)})
            i += len(sep)
        return out

    def __call__(self, x, grouped=None):
        """x [B, H, W, in_channels] bf16 -> (head, shared): the head tensor (layout: task_offsets()) and the shared conv's output
        [B, H, W, 64] (construct's (ret_dicts, x), center_head.py:193-200)."""
        if grouped if grouped is not None else SEPHEAD_GROUPED:
            return self.forward_mid(x)[:2]
        sh = self.shared_conv(x)
        mid = nn_ops.conv2d(sh, self._first)                                    # [B, H, W, 64 x branches]
        B, H, W, _ = sh.shape
        br = self.branches()
        head = torch.empty((B, H, W, 8 * len(br)), dtype=torch.bfloat16, device=x.device)
        for i, (_, _, _, c2) in enumerate(br):
            nn_ops.conv2d(mid, c2.packed, out=head, c_off=8 * i, x_c_off=64 * i)
        return head, sh

    def forward_mid(self, x):
        """the three launches of the fast form -> (head, shared, mid): mid [B, H, W, 64 x branches] bf16 is the merged first convs'
        output, the tensor the grouped conv reads (a training step differentiates through it)"""
        sh = self.shared_conv(x)
        mid = nn_ops.conv2d(sh, self._first)                                    # [B, H, W, 64 x branches]
        B, H, W, _ = sh.shape
        head = torch.empty((B, H, W, (self.head_channels + 7) // 8 * 8), dtype=torch.bfloat16, device=x.device)
        nn_ops.conv2d_grouped(mid, self._second, head)
        return head, sh, mid

    def loss(self, example, head, grad=False):
        """center_head.py:208-271 on the head tensor of __call__ (raw logits in the layout of task_offsets(); the per-branch A/B layout
        of MD_SEPHEAD_GROUPED=0 is 8 channels per branch wide, which at six tasks is past the operator's 160 channels):
        example = the dict of det_ops.cp_assign_targets -> the dict of det_ops.cp_loss (total, parts, num_pos[, grad]); the
        differentiable form is det_ops.center_point_loss(head, example, self.loss_op())."""
        return self.loss_op()(head, example, grad=grad)

    def loss_op(self):
        return self._lazy("loss", lambda: det_ops.CenterPointLoss.from_head(self))


@DETECTORS.register_module
class PointPillars(Module):
    """det3d's PointPillars detector with a CenterHead (centerpoint/det3d_ms/models/detectors/point_pillars.py; the nuScenes
    CenterPoint-PP config): neck (graphs.RPN) -> bbox_head (CenterHead) -> one CenterHeadPost per task -> the task merge of
    tools_ms/eval.py:84-111 (merge_center_tasks); cp_post=True (default: the MD_CP_POST setting) and return_aux=False: the
    post-processing of every task and the merge as one chain (det_ops.CenterHeadPostBatched), the same result.  The pillar encoder (reader) and the scatter
    (backbone) are out of scope: forward() takes the scattered pseudo-image [B, H, W, 64] bf16."""

    def __init__(self, neck, bbox_head, reader=None, backbone=None, train_cfg=None, test_cfg=None, pretrained=None, seed=7,
                 cp_post=None):
        if reader is not None or backbone is not None:
            raise ValueError("PointPillars: the pillar encoder (`reader`) and the scatter (`backbone`) are not part of this build; "
                             "drop them from the config and feed the scattered pseudo-image [B, H, W, 64] bf16 to forward()")
        _split_forward_of(self, test_cfg)
        self.neck = build_neck(dict(neck, seed=seed) if isinstance(neck, dict) and "seed" not in neck else neck)
        self.bbox_head = build_head(dict(bbox_head, seed=seed + 1) if isinstance(bbox_head, dict) and "seed" not in bbox_head else bbox_head)
        self.test_cfg = test_cfg
        self.train_cfg = dict(train_cfg) if train_cfg else None
        self.max_per_task = int(test_cfg["nms"]["nms_post_max_size"])
        self.cp_post = CP_POST if cp_post is None else bool(cp_post)

    def children(self):
        return [self.neck, self.bbox_head]

    def post_batched(self):
        return self._lazy("post_batched", lambda: det_ops.CenterHeadPostBatched(self.bbox_head.task_offsets(), self.bbox_head.num_classes,
                                                                               self.test_cfg))

    def forward(self, pseudo_image, return_aux=False):
        """pseudo_image [B, H, W, 64] bf16 -> (dets [B, tasks x nms_post_max_size, 11] f32, count [B] i32): per row the 9 box values
        (x, y, z, dx, dy, dz, vx, vy, rot), score, label over all tasks; rows past count are zero."""
        feat = self.neck(pseudo_image)
        head, shared = self.bbox_head(feat)
        if self.cp_post and not return_aux:
            return self.post_batched()(head)
        posts = [det_ops.CenterHeadPost(off, nc, self.test_cfg)
                 for off, nc in zip(self.bbox_head.task_offsets(), self.bbox_head.num_classes)]
        outs = [post(head) for post in posts]
        dets, count = merge_center_tasks(outs, self.bbox_head.num_classes, self.max_per_task)
        if return_aux:
            return (dets, count), dict(neck=feat, head=head, shared=shared, tasks=outs)
        return dets, count

    __call__ = forward

    def loss(self, pseudo_image, example, grad=False):
        """the neck and the head, then CenterHead.loss on the head tensor: example = the dict of det_ops.cp_assign_targets -> the dict of
        det_ops.cp_loss (grad=True: with d total / d head, the first gradient of a training step)"""
        head, _ = self.bbox_head(self.neck(pseudo_image))
        return self.bbox_head.loss(example, head, grad=grad)

    def head_trainer(self, optimizer_cfg=None):
        """CenterHead.head_trainer of the model's head; optimizer_cfg: None = train_cfg["optimizer"] (none there:
        optim.CENTERPOINT_OPTIMIZER)"""
        return self.bbox_head.head_trainer(optimizer_cfg, fallback=(self.train_cfg or {}).get("optimizer"))

    def train_step(self, pseudo_image, example, lr, beta1=0.9):
        """One training step of the head on a batch (the neck frozen): pseudo_image [B, H, W, 64] bf16, example = the dict of
        det_ops.cp_assign_targets -> the dict of loss(grad=True) (the loss BEFORE the update) plus `neck`, `head`, `shared`, `mid` and
        `dmid` (optim.CenterPointHeadTrainer.train_step).  Nothing is read back."""
        feat = self.neck(pseudo_image)
        return dict(self.head_trainer().train_step(feat, example, lr, beta1), neck=feat)

    def evaluate_nusc(self, dets, count, poses, gt_records, ego_translations):
        """The nuScenes detection result (detection_cvpr_2019) of forward()'s rows (dets [B, max_det, 11], count [B]) for the B samples
        of ego_translations, on the device: nusc_eval.PackedNusc.add_dets takes the rows as they lie (md_nusc_rows: the global frame,
        the attribute rule, the class-range filter and the grouping, no host copy), md_nusc_eval_match and md_nusc_eval_accumulate fill
        the curves, NuscDetectionEval.summarize() reads them.  poses: per sample cs_rotation, cs_translation, ego_rotation,
        ego_translation (nusc_eval.pose_array); the class names are the config's `tasks` in order.
        -> what NuscDetectionEval(gt_records, rows_to_results' records, ...).summarize() returns on the same rows."""
        from . import nusc_eval

        names = [n for task in self.bbox_head.class_names for n in task]
        packed = nusc_eval.pack_nusc(gt_records, ego_translations, names, device=dets.device).add_dets(dets, count, poses, 0)
        return nusc_eval.NuscDetectionEval.from_packed(packed).evaluate(backend="device").summarize()


def merge_center_tasks(outs, num_classes, max_per_task):
    """The task merge of tools_ms/eval.py:84-111 on the device: per sample and task the first size rows, size = the rows among the first
    count whose score is > 0; tasks concatenated in order, each label shifted by the summed num_class of the earlier tasks.
    outs: per task (boxes [B, k, 9], scores [B, k], labels [B, k], count [B]) -> (dets [B, T x max_per_task, 11] f32, count [B] i32)."""
    B, dev, m = outs[0][1].shape[0], outs[0][1].device, int(max_per_task)
    T = len(outs)
    rows = torch.zeros((B, T * m + 1, 11), dtype=torch.float32, device=dev)      # the last row takes the rows that are dropped
    j = torch.arange(m, device=dev).view(1, m)
    base = torch.zeros((B, 1), dtype=torch.int64, device=dev)
    flag = 0
    for (boxes, scores, labels, count), nc in zip(outs, num_classes):
        sc = scores[:, :m]
        size = ((j < count.view(B, 1).long()) & (sc > 0)).sum(1, keepdim=True)
        r = torch.cat([boxes[:, :m], sc.unsqueeze(2), (labels[:, :m] + flag).to(torch.float32).unsqueeze(2)], 2)
        dst = torch.where(j < size, base + j, torch.full_like(j, T * m))
        rows.scatter_(1, dst.unsqueeze(2).expand(B, m, 11), r)
        base = base + size
        flag += int(nc)
    rows[:, T * m] = 0
    return rows[:, :T * m].contiguous(), base.view(B).to(torch.int32)


# ----------------------------------------------------------------------------- point-cloud front end (csrc/pillars.hip)
@READERS.register_module
class PillarFeatureNet(Module):
    """centerpoint/det3d_ms/models/readers/pillar_encoder.py:70-199: the decoration of every point with its offsets from the voxel's
    mean and from the pillar centre, then the PFN layers (:18-67) -- Dense without bias + BatchNorm(eps 1e-3) + ReLU + max over the
    voxel's rows, a non-last layer (units = filters / 2) concatenating the maximum to every row.  Parameters in the reference's layout
    (`layers[i] = (weight [units, in], (gamma, beta, mean, var, eps))`); to() folds them (det_ops.pack_pfn).  The net only runs fused
    with the scatter: PointPillarsScatter.__call__ makes the one md_pillar_encode launch."""

    def __init__(self, num_input_features=4, num_filters=(64,), with_distance=False, voxel_size=(0.2, 0.2, 4),
                 pc_range=(0, -40, -3, 70.4, 40, 1), norm_cfg=None, virtual=False, seed=7):
        num_filters = [int(c) for c in num_filters]
        if with_distance or virtual:
            raise ValueError("PillarFeatureNet: with_distance=True and virtual=True are not built")
        if int(num_input_features) not in (4, 5) or num_filters not in ([64], [64, 64]):
            raise ValueError(f"PillarFeatureNet: built for 4 or 5 point features and num_filters (64,) or (64, 64), got "
                             f"num_input_features={num_input_features}, num_filters={tuple(num_filters)}")
        eps = (norm_cfg or {}).get("eps", 1e-3)
        if eps != 1e-3:
            raise ValueError("PillarFeatureNet: the reference's PFN layers use BatchNorm eps 1e-3 whatever norm_cfg says")
        init = ParamInit(seed)
        self.num_input_features, self.num_filters = int(num_input_features), num_filters
        self.vx, self.vy = float(voxel_size[0]), float(voxel_size[1])
        self.x_offset, self.y_offset = self.vx / 2 + float(pc_range[0]), self.vy / 2 + float(pc_range[1])
        self.layers = []
        cin = self.num_input_features + 5
        for i, c in enumerate(num_filters):
            units = c if i == len(num_filters) - 1 else c // 2
            w = init.conv(units, cin, 1, std=math.sqrt(2.0 / cin)).reshape(units, cin)
            gamma, beta, mean, var, _ = init.bn(units, eps)
            beta = init.bias(units, std=0.1)               # both signs: where the shift is positive the padded rows win the maximum
            self.layers.append((w, (gamma, beta, mean, var, eps)))
            cin = 2 * units
        self.out_channels = num_filters[-1]

    def _derive(self, device):
        self.packed = det_ops.pack_pfn(self.layers).to(device)


@BACKBONES.register_module
class PointPillarsScatter(Module):
    """pillar_encoder.py:202-228: the voxel features scattered to the dense BEV canvas.  Here the canvas is written by the same launch
    that computes the features, in the NHWC layout the neck reads (the reference's transpose to NCHW is not needed)."""

    def __init__(self, num_input_features=64, norm_cfg=None, name="PointPillarsScatter", ds_factor=1, **kwargs):
        if int(ds_factor) != 1 or int(num_input_features) != 64:
            raise ValueError(f"PointPillarsScatter: built for ds_factor=1 and 64 channels, got ds_factor={ds_factor}, "
                             f"num_input_features={num_input_features}")
        self.nchannels = 64

    def __call__(self, reader, voxels, coors, num_points, voxel_num, hw):
        """md_voxelize's outputs -> pseudo-image [B, H, W, 64] bf16"""
        return det_ops.pillar_encode(voxels, num_points, coors, voxel_num, reader.packed, hw, reader.vx, reader.vy, reader.x_offset,
                                     reader.y_offset)


@DETECTORS.register_module
class PillarDetector(Module):
    """CenterPoint-PP from raw points (det3d's PointPillars detector with its reader and backbone,
    centerpoint/det3d_ms/models/detectors/point_pillars.py): voxel generator (md_voxelize) -> PillarFeatureNet + PointPillarsScatter
    (md_pillar_encode) -> graphs.PointPillars (neck, bbox_head, post-processing, unchanged).  Everything stays on the device: the
    outputs have fixed capacity and no size is read back."""

    def __init__(self, reader, backbone, neck, bbox_head, voxel_generator, train_cfg=None, test_cfg=None, pretrained=None, seed=7,
                 sweeps=None):
        from .registry import build
        self.reader = build(dict(reader, seed=seed + 2) if isinstance(reader, dict) and "seed" not in reader else reader, READERS)
        self.backbone = build_backbone(backbone)
        self.detector = PointPillars(neck, bbox_head, train_cfg=train_cfg, test_cfg=test_cfg, pretrained=pretrained, seed=seed)
        vg = dict(voxel_generator)
        self.pc_range = tuple(float(v) for v in vg["range"])
        self.voxel_size = tuple(float(v) for v in vg["voxel_size"])
        self.max_points, self.max_voxels = int(vg["max_points_in_voxel"]), int(vg["max_voxel_num"])
        gx, gy, gz = det_ops.voxel_grid(self.voxel_size, self.pc_range)
        if gz != 1:
            raise ValueError(f"PillarDetector: pillars span the whole z range (one cell), the voxel generator gives {gz}")
        self.grid_hw = (gy, gx)
        if (self.reader.vx, self.reader.vy) != self.voxel_size[:2] or self.reader.num_filters[-1] != self.backbone.nchannels:
            raise ValueError("PillarDetector: the reader's voxel_size / width do not match the voxel generator / the backbone")
        self.train_cfg = dict(train_cfg) if train_cfg else None
        self._voxel_generator = vg
        self._sweeps_cfg = dict(sweeps) if sweeps else None

    def children(self):
        return [self.reader, self.backbone, self.detector]

    @property
    def neck(self):
        return self.detector.neck

    @property
    def bbox_head(self):
        return self.detector.bbox_head

    def pseudo_image(self, points, offsets):
        """points [N, F] f32, offsets [B + 1] i32 -> (canvas [B, H, W, 64] bf16, (voxels, coors, num_points, voxel_num))"""
        vox = det_ops.voxelize(points, offsets, self.voxel_size, self.pc_range, self.max_points, self.max_voxels)
        voxels, coors, num_points, voxel_num = vox
        return self.backbone(self.reader, voxels, coors, num_points, voxel_num, self.grid_hw), vox

    def forward(self, points, offsets, return_aux=False):
        """points [N, F] f32: the B samples' points back to back; offsets [B + 1] i32 (device) ->
        (dets [B, tasks x nms_post_max_size, 11] f32, count [B] i32) as PointPillars.forward"""
        if points.shape[1] != self.reader.num_input_features:
            raise ValueError(f"PillarDetector: the reader takes {self.reader.num_input_features} point features, got {points.shape[1]}")
        canvas, (voxels, coors, num_points, voxel_num) = self.pseudo_image(points, offsets)
        if return_aux:
            out, aux = self.detector.forward(canvas, return_aux=True)
            return out, dict(aux, voxels=voxels, coors=coors, num_points=num_points, voxel_num=voxel_num, pseudo_image=canvas)
        return self.detector.forward(canvas)

    __call__ = forward

    def sweeps_op(self):
        """det_ops.SweepMerger with the model's `sweeps` (nsweeps, min_distance, order; configs/centerpoint/centerpoint_pp_nusc_sweeps.py)"""
        if not self._sweeps_cfg:
            raise ValueError("PillarDetector: the model has no `sweeps` (see configs/centerpoint/centerpoint_pp_nusc_sweeps.py)")
        return self._lazy("sweeps", lambda: det_ops.SweepMerger(**self._sweeps_cfg))

    def merge_sweeps(self, points, lengths, matrices, time_lags, order=None, begins=None, return_status=False):
        """The reference loader's multi-sweep step on the device (det_ops.SweepMerger: read_sweep per past sweep and the concatenation):
        points [N, 4 or 5] f32 = the pool that holds every frame of the B samples; lengths, matrices, time_lags [B][nsweeps] (frame 0
        the key frame; a matrix None = no transform), order = the loader's draw -> (points [N, 5] f32, offsets [B + 1] i32) as forward
        and train_example take them (zero rows behind offsets[B]); nothing is read back.  return_status=True: plus status [B] i32."""
        pts, offsets, status = self.sweeps_op()(points, lengths, matrices, time_lags, order=order, begins=begins)
        return (pts, offsets, status) if return_status else (pts, offsets)

    def forward_sweeps(self, points, lengths, matrices, time_lags, order=None, begins=None, return_aux=False):
        """merge_sweeps, then forward on the merged cloud"""
        pts, offsets = self.merge_sweeps(points, lengths, matrices, time_lags, order=order, begins=begins)
        return self.forward(pts, offsets, return_aux=return_aux)

    def evaluate_nusc(self, dets, count, poses, gt_records, ego_translations):
        """The nuScenes detection result of forward()'s rows on the device, beside PointPillarsKITTIPoints.evaluate_kitti:
        PointPillars.evaluate_nusc of the inner detector (class names from the config's `tasks`)."""
        return self.detector.evaluate_nusc(dets, count, poses, gt_records, ego_translations)

    TRAIN_CFG_HINT = "configs/centerpoint/centerpoint_pp_nusc_train.py"

    def augment_op(self):
        """det_ops.CenterPointAugment with train_cfg["augment"] on this model's range"""
        r = self.pc_range
        return self._lazy("augment", lambda: det_ops.CenterPointAugment((r[0], r[1], r[3], r[4]), **dict(self._train_cfg("augment"))))

    def targets_op(self):
        """det_ops.CenterPointTargets with train_cfg["assigner"] on this model's voxel generator"""
        return self._lazy("targets", lambda: det_ops.CenterPointTargets(self._train_cfg("assigner"), self._voxel_generator))

    def _train_canvas(self, points, offsets):
        # the reference trains with its own voxel budget (30 000 on nuScenes, 60 000 in evaluation)
        max_voxels = int((self.train_cfg or {}).get("max_voxel_num", self.max_voxels))
        voxels, coors, num_points, voxel_num = det_ops.voxelize(points, offsets, self.voxel_size, self.pc_range, self.max_points, max_voxels)
        return self.backbone(self.reader, voxels, coors, num_points, voxel_num, self.grid_hw)

    def loss(self, points, offsets, example, grad=False):
        """the voxeliser (with train_cfg["max_voxel_num"] where given) and the pillar encoder, then PointPillars.loss on the canvas:
        example = the dict of det_ops.cp_assign_targets -> the dict of det_ops.cp_loss (grad=True: with d total / d head)"""
        if points.shape[1] != self.reader.num_input_features:
            raise ValueError(f"PillarDetector: the reader takes {self.reader.num_input_features} point features, got {points.shape[1]}")
        return self.detector.loss(self._train_canvas(points, offsets), example, grad=grad)

    def train_example(self, points, offsets, gt_boxes, gt_classes, gt_count, generator=None, draws=None, sampled=None):
        """Raw points and ground truth -> the `example` of loss(), on the device with nothing read back: the training branch of the
        reference's Preprocess and the ground-truth filter of its Voxelization (det_ops.CenterPointAugment: points [N,5] f32, offsets
        [B+1] i32, gt_boxes [B,G,9] f32, gt_classes [B,G] global 1-based class or 0, gt_count [B]; sampled = the drawn database
        candidates, draws = global [B,7] f64 of its draw(), None: drawn with `generator`), then AssignLabel
        (det_ops.CenterPointTargets) on the fixed-capacity box list, whose rows behind the sample's count are class 0, i.e. padding.
        -> the dict of det_ops.cp_assign_targets plus augment = the dict of CenterPointAugment."""
        a = self.augment_op()(points, offsets, gt_boxes, gt_classes, gt_count, sampled=sampled, draws=draws, generator=generator)
        tg = self.targets_op()
        if a["gt_boxes"].shape[1] > tg.max_objs:
            raise ValueError(f"PillarDetector: G + S = {a['gt_boxes'].shape[1]} rows exceed max_objs = {tg.max_objs}")
        return dict(tg(a["gt_boxes"], a["gt_classes"]), augment=a)

    def train_loss(self, points, offsets, gt_boxes, gt_classes, gt_count, generator=None, draws=None, sampled=None, grad=False):
        """train_example, then loss() on the augmented points: raw points + ground truth -> loss (and, grad=True, d total / d head)
        as one device chain.  -> the dict of loss() plus `example`."""
        ex = self.train_example(points, offsets, gt_boxes, gt_classes, gt_count, generator=generator, draws=draws, sampled=sampled)
        return dict(self.loss(ex["augment"]["points"], ex["augment"]["offsets"], ex, grad=grad), example=ex)

    def head_trainer(self, optimizer_cfg=None):
        """PointPillars.head_trainer of the inner detector (optimizer_cfg None: train_cfg["optimizer"], which the detector got too)"""
        return self.detector.head_trainer(optimizer_cfg)

    def train_step(self, points, offsets, gt_boxes, gt_classes, gt_count, lr, beta1=0.9, generator=None, draws=None, sampled=None):
        """train_example, then one step of head_trainer() on the augmented points: raw points + ground truth -> updated head as one
        device chain (reader, backbone, neck and shared conv frozen).  -> the dict of PointPillars.train_step plus `example`."""
        ex = self.train_example(points, offsets, gt_boxes, gt_classes, gt_count, generator=generator, draws=draws, sampled=sampled)
        self.head_trainer()
        canvas = self._train_canvas(ex["augment"]["points"], ex["augment"]["offsets"])
        return dict(self.detector.train_step(canvas, ex, lr, beta1), example=ex)


# ----------------------------------------------------------------------------- PointPillars, anchor-based (KITTI)
class PPAnchorHead(Module):
    """conv_cls / conv_box / conv_dir_cls of the KITTI RPN (pointpillars/src/pointpillars.py:562-578): three 1x1 convs with bias, no
    BatchNorm, no activation, on the neck's concatenated features.  The three ConvModules are the source of truth; to() builds ONE
    md_conv2d launch from them (merged_conv) whose output [B, H, W, roundup(A K + 7 A + 2 A, 8)] bf16 holds the three side by side:
    the head tensor md_pp_scores and md_pp_decode_selected read in place (head_offsets())."""

    def __init__(self, init, in_channels, num_anchors, num_classes, use_direction_classifier=True):
        self.A, self.K = int(num_anchors), int(num_classes)
        kw = dict(bn=False, relu=False, bias=True)
        self.conv_cls = ConvModule(init, in_channels, self.A * self.K, 1, **kw)
        self.conv_box = ConvModule(init, in_channels, self.A * 7, 1, **kw)
        self.conv_dir_cls = ConvModule(init, in_channels, self.A * 2, 1, **kw) if use_direction_classifier else None
        self.head_channels = sum(m.cout for m in self.children())

    def children(self):
        return [m for m in (self.conv_cls, self.conv_box, self.conv_dir_cls) if m is not None]

    _merged = None      # the three convs as one pack (_derive): what optim.HeadTrainer (PointPillarsNet.head_trainer) trains

    def _derive(self, device):
        self._merged = merged_conv(self.children(), device)

    def head_offsets(self):
        """first channel of each conv's outputs in the head tensor; dir_cls None without a direction classifier"""
        return dict(cls=0, box=self.conv_cls.cout, dir_cls=self.conv_cls.cout + self.conv_box.cout if self.conv_dir_cls is not None else None)

    def __call__(self, x):
        return nn_ops.conv2d(x, self._merged)


@DETECTORS.register_module(name="PointPillarsKITTI")
class PointPillarsNet(Module):
    """Registered as "PointPillarsKITTI" (a config's `type`); the class keeps the reference's name.  The reference's KITTI PointPillars from the scattered pseudo-image on (pointpillars/src/pointpillars.py:655-800, inference):
    the RPN of :367-621 -- graphs.RPN with block1's inner BatchNorms at the framework's default eps 1e-5 (:470), every other one at
    1e-3 -- the three 1x1 heads as one launch (PPAnchorHead) and det_ops.PPHeadPost on the head tensor.  The anchors come from the
    config's anchor generators (det_ops.generate_anchors at the feature-map size) and are a device constant.
    This type starts at the pseudo-image and refuses `voxel_feature_extractor` / `middle_feature_extractor` (ValueError): the model's
    reader and scatter (a tenth point feature, the z offset from the pillar centre, and an fp16 Dense: md_pp_pillar_encode) belong to
    graphs.PointPillarsKITTIPoints, which wraps this class.  Not built: use_bev=True, encode_background_as_zeros=False,
    use_self_train=False."""

    def __init__(self, rpn, voxel_generator, anchor_generators, num_class=1, use_direction_classifier=True,
                 encode_background_as_zeros=True, use_sigmoid_score=True, use_bev=False, use_self_train=True, anchor_area_threshold=1,
                 voxel_feature_extractor=None, middle_feature_extractor=None, class_names=None, train_cfg=None, test_cfg=None,
                 pretrained=None, seed=7):
        if voxel_feature_extractor is not None or middle_feature_extractor is not None:
            raise ValueError("PointPillarsNet: this type starts at the scattered pseudo-image [B, H, W, 64] bf16; a config with "
                             "`voxel_feature_extractor` / `middle_feature_extractor` is built by type \"PointPillarsKITTIPoints\", which "
                             "runs the reader (a tenth point feature and an fp16 Dense: md_pp_pillar_encode) from raw points")
        if use_bev:
            raise ValueError("PointPillarsNet: use_bev=True (the BEV extractor branch of the RPN) is not built")
        if not encode_background_as_zeros or not use_sigmoid_score:
            raise ValueError("PointPillarsNet: only encode_background_as_zeros=True with sigmoid scores is built")
        if not use_self_train:
            raise ValueError("PointPillarsNet: use_self_train=False (the limit_period direction form) is not built")
        if not test_cfg:
            raise ValueError("PointPillarsNet: test_cfg with nms_pre_max_size, nms_post_max_size, nms_score_threshold and "
                             "nms_iou_threshold is required")
        _split_forward_of(self, test_cfg)
        rpn, vg = dict(rpn), dict(voxel_generator)
        strides, ups = [int(s) for s in rpn.get("layer_strides", (2, 2, 2))], [int(s) for s in rpn.get("upsample_strides", (1, 2, 4))]
        if len(strides) != 3 or len(ups) != 3 or any(int(np.prod(strides[:i + 1])) * ups[0] != strides[0] * ups[i] for i in range(3)):
            raise ValueError(f"PointPillarsNet: the three deblocks must reach one size, got layer_strides {strides}, upsample_strides {ups}")
        self.in_channels = int(rpn.get("num_input_filters", 64))
        self.neck = RPN(layer_nums=rpn.get("layer_nums", (3, 5, 5)), ds_layer_strides=strides,
                        ds_num_filters=rpn.get("num_filters", (64, 128, 256)), us_layer_strides=ups,
                        us_num_filters=rpn.get("num_upsample_filters", (128, 128, 128)), num_input_features=self.in_channels,
                        norm_cfg=dict(eps=1e-3), inner_norm_eps=(1e-5, None, None), seed=seed)
        self.generators = [g if isinstance(g, det_ops.AnchorGeneratorStride) else
                           det_ops.AnchorGeneratorStride(sizes=g["sizes"], anchor_strides=g["strides"], anchor_offsets=g["offsets"],
                                                         rotations=g["rotations"], match_threshold=g.get("matched_threshold", -1),
                                                         unmatch_threshold=g.get("unmatched_threshold", -1),
                                                         anchor_range=vg["point_cloud_range"]) for g in anchor_generators]
        self.num_class = int(num_class)
        self.num_anchors = sum(g.num_anchors_per_localization for g in self.generators)
        self.bbox_head = PPAnchorHead(ParamInit(seed + 1), self.neck.out_channels, self.num_anchors, self.num_class,
                                      use_direction_classifier)
        self.pc_range = tuple(float(v) for v in vg["point_cloud_range"])
        self.voxel_size = tuple(float(v) for v in vg["voxel_size"])
        gx, gy, _ = det_ops.voxel_grid(self.voxel_size, self.pc_range)
        self.grid_hw = (gy, gx)                                              # the pseudo-image
        # block1's first conv (3x3, pad 1, stride s) gives (n - 1) // s + 1 cells, its deblock multiplies by the upsample stride
        self.feature_hw = (((gy - 1) // strides[0] + 1) * ups[0], ((gx - 1) // strides[0] + 1) * ups[0])
        self.anchor_area_threshold = float(anchor_area_threshold)
        self.class_names = list(class_names) if class_names is not None else None
        self.test_cfg = dict(test_cfg)
        self.train_cfg = dict(train_cfg) if train_cfg else None
        off = self.bbox_head.head_offsets()
        self.post = det_ops.PPHeadPost(dict(num_anchors=self.num_anchors, num_classes=self.num_class, off_cls=off["cls"], off_box=off["box"],
                                            off_dir=off["dir_cls"], use_self_train=use_self_train,
                                            **{k: self.test_cfg[k] for k in ("nms_pre_max_size", "nms_post_max_size", "nms_score_threshold",
                                                                             "nms_iou_threshold")}))

    def children(self):
        return [self.neck, self.bbox_head]

    def head_offsets(self):
        return self.bbox_head.head_offsets()

    def to(self, device):
        super().to(device)
        fh, fw = self.feature_hw
        self.anchors = det_ops.generate_anchors(self.generators, (1, fh, fw), device=device)["anchors"].reshape(-1, 7)
        self.anchors_bv = det_ops.rbbox2d_to_near_bbox(self.anchors[:, [0, 1, 3, 4, 6]])
        return self

    def anchors_mask_from_coors(self, coors, voxel_num=None):
        """coors [B, MV, 4] i32 (b, z, y, x: md_voxelize's output) or a list of per-sample [V, 3] (z, y, x), voxel_num [B] (rows that
        count; None = all) -> the anchors mask [B, N] uint8: det_ops.anchors_mask per sample with anchor_area_threshold, as
        data/preprocess.py:211-225 does.  Pre-processing: reads voxel_num on the host."""
        nums = None if voxel_num is None else [int(v) for v in voxel_num.tolist()]
        rows = []
        for b in range(len(coors)):
            c = coors[b][:, -3:] if nums is None else coors[b][:nums[b], -3:]
            _, m = det_ops.anchors_mask(c.contiguous(), (self.grid_hw[1], self.grid_hw[0]), self.anchors_bv, self.voxel_size, self.pc_range,
                                        self.anchor_area_threshold)
            rows.append(m.to(torch.uint8))
        return torch.stack(rows)

    def forward(self, pseudo_image, anchors_mask=None, return_aux=False):
        """pseudo_image [B, H, W, 64] bf16, anchors_mask [B, N] or None (all valid) -> (dets [B, nms_post_max_size, 9] f32 = x, y, z,
        w, l, h, rot, score, label; count [B] i32); rows past count are zero.  Nothing is read back to the host."""
        if isinstance(pseudo_image, (tuple, list)):       # (pseudo_image, anchors_mask): the form forward_streams hands to SplitForward
            pseudo_image, anchors_mask = pseudo_image
        if tuple(pseudo_image.shape[1:]) != (self.grid_hw[0], self.grid_hw[1], self.in_channels):
            raise ValueError(f"PointPillarsNet: the pseudo-image is [B, {self.grid_hw[0]}, {self.grid_hw[1]}, {self.in_channels}], got "
                             f"{tuple(pseudo_image.shape)}")
        feat = self.neck(pseudo_image)
        head = self.bbox_head(feat)
        B = head.shape[0]
        n = self.anchors.shape[0]
        seg = self.const(("segments", B), lambda: _segments(B, n, head.device))
        if return_aux:
            out, aux = self.post(head, self.anchors, anchors_mask, segments=seg, return_aux=True)
            return out, dict(aux, neck=feat, head=head)
        return self.post(head, self.anchors, anchors_mask, segments=seg)

    __call__ = forward

    def forward_streams(self, pseudo_image, anchors_mask=None):
        """forward() through test_cfg.streams HIP streams (SplitForward): the mask is split with the batch"""
        if anchors_mask is None:
            return self.forward_split(pseudo_image)
        return self.forward_split((pseudo_image, anchors_mask), prepare=lambda p, m: (p, m))

    def loss_op(self):
        """det_ops.PointPillarsLoss of this head's layout with the settings of train_cfg (None: the KITTI configurations' values)"""
        return self._lazy("loss", lambda: det_ops.PointPillarsLoss.from_net(self, self.train_cfg))

    def loss(self, pseudo_image, example, grad=False):
        """PointPillarsWithLossCell.construct (pointpillars/src/pointpillars.py:817-872): the neck and the head, then the loss on the head
        tensor.  example = dict(labels [B,N] i32, reg_targets [B,N,7] f32), the first two outputs of det_ops.assign_targets_batch on
        self.anchors -> the dict of det_ops.pp_loss (grad=True: with d total / d head, the first gradient of a training step) plus
        `head`, the tensor the gradient belongs to; the differentiable form is det_ops.point_pillars_loss(head, ..., self.loss_op())."""
        head = self.bbox_head(self.neck(pseudo_image))
        out = self.loss_op()(head, example["labels"], example["reg_targets"], self.anchors, grad=grad)
        return dict(out, head=head)

    def head_trainer(self, optimizer_cfg=None):
        """optim.HeadTrainer of this model's head (the three 1x1 convs, the neck frozen): train_step(pseudo_image, example, lr, beta1)
        continues loss(grad=True) through md_conv1x1_bwd_weight, md_grad_sumsq and md_adam_step on the device.  optimizer_cfg: None =
        train_cfg["optimizer"] (none there: optim.DEFAULT_OPTIMIZER).  One trainer per head: a call without a config returns the
        existing one, a call with one replaces it (fresh moments).  The model has to be on its device."""
        from . import optim

        head = self.bbox_head
        return head._head_trainer(optim.HeadTrainer, self, optimizer_cfg, (self.train_cfg or {}).get("optimizer"),
                                  lambda: head._derive(head._merged.w.device))


# ----------------------------------------------------------------------------- PointPillars (KITTI) from raw points (csrc/ppreader.hip)
@READERS.register_module
class PPPillarFeatureNet(Module):
    """The KITTI model's PillarFeatureNet (pointpillars/src/pointpillars.py:226-317) with its one PFNLayer (:180-223): every point
    decorated with its offsets from the voxel's mean and from the pillar centre in x, y AND z (ten features, eleven with_distance),
    then Dense without bias under to_float(float16) + BatchNorm(eps 1e-3) + ReLU + max over the voxel's rows.  Parameters in the
    reference's layout (`layers[0] = (weight [64, K], (gamma, beta, mean, var, 1e-3))`); to() keeps the raw weight and folds the
    BatchNorm into scale / shift (det_ops.pack_pp_pfn).  The net only runs fused with the scatter, as one md_pp_pillar_encode launch."""

    def __init__(self, num_input_features=4, use_norm=True, num_filters=(64,), with_distance=False, voxel_size=(0.16, 0.16, 4),
                 pc_range=(0, -39.68, -3, 69.12, 39.68, 1), seed=7):
        num_filters = [int(c) for c in num_filters]
        if not use_norm:
            raise ValueError("PPPillarFeatureNet: use_norm=False (a Dense with bias and no BatchNorm) is not built")
        if num_filters != [64]:
            raise ValueError(f"PPPillarFeatureNet: built for one PFN layer, num_filters (64,), got {tuple(num_filters)}")
        if int(num_input_features) != 4:
            raise ValueError(f"PPPillarFeatureNet: built for 4 point features (x, y, z, r), got {num_input_features}")
        init = ParamInit(seed)
        self.num_input_features, self.num_filters, self.with_distance = 4, num_filters, bool(with_distance)
        self.voxel_size = tuple(float(v) for v in voxel_size[:3])
        self.offsets = tuple(float(v) / 2 + float(lo) for v, lo in zip(voxel_size[:3], pc_range[:3]))
        K = 10 + int(self.with_distance)
        w = init.conv(64, K, 1, std=math.sqrt(2.0 / K)).reshape(64, K)
        gamma, _, mean, var, _ = init.bn(64, 1e-3)
        gamma = torch.from_numpy(init.rng.uniform(0.5, 1.5, 64).astype(np.float32))
        beta = init.bias(64, std=0.1)                      # both signs: where the shift is positive the padded rows win the maximum
        self.layers = [(w, (gamma, beta, mean, var, 1e-3))]
        self.out_channels = 64

    def _derive(self, device):
        self.packed = det_ops.pack_pp_pfn(self.layers).to(device)


@DETECTORS.register_module(name="PointPillarsKITTIPoints")
class PointPillarsKITTIPoints(Module):
    """The KITTI PointPillars from raw points, built from the reference's config keys: voxel generator (md_voxelize) ->
    PillarFeatureNet + PointPillarsScatter (md_pp_pillar_encode) -> the anchor mask of the batch (md_pp_anchor_mask) -> an unchanged
    graphs.PointPillarsNet, i.e. PointPillarsNet.construct(voxels, num_points, coors, anchors, anchors_mask)
    (pointpillars/src/pointpillars.py:728-739) with the data pipeline's voxeliser and mask in front.  Everything stays on the device:
    the outputs have fixed capacity and no size is read back."""

    def __init__(self, voxel_generator, voxel_feature_extractor=None, middle_feature_extractor=None, num_point_features=4, use_norm=True,
                 seed=7, **kwargs):
        vg = dict(voxel_generator)
        self.inner = PointPillarsNet(voxel_generator=vg, seed=seed, **kwargs)
        vfe = dict(voxel_feature_extractor or {})
        unknown = set(vfe) - {"num_filters", "with_distance", "type"} | set(dict(middle_feature_extractor or {})) - {"type"}
        if unknown:
            raise ValueError(f"PointPillarsKITTIPoints: options that are not built: {sorted(unknown)}")
        self.max_points, self.max_voxels = int(vg["max_number_of_points_per_voxel"]), int(vg["max_number_of_voxels"])
        if self.max_points > 32:
            raise ValueError(f"PointPillarsKITTIPoints: at most 32 points per voxel are built, got {self.max_points}")
        self.pc_range, self.voxel_size = self.inner.pc_range, self.inner.voxel_size
        gx, gy, gz = det_ops.voxel_grid(self.voxel_size, self.pc_range)
        if gz != 1:
            raise ValueError(f"PointPillarsKITTIPoints: pillars span the whole z range (one cell), the voxel generator gives {gz}")
        self.grid_hw = self.inner.grid_hw
        self.reader = PPPillarFeatureNet(num_input_features=num_point_features, use_norm=use_norm, num_filters=vfe.get("num_filters", (64,)),
                                         with_distance=vfe.get("with_distance", False), voxel_size=self.voxel_size,
                                         pc_range=self.pc_range, seed=seed + 2)
        if self.reader.out_channels != self.inner.in_channels:
            raise ValueError("PointPillarsKITTIPoints: the reader's width does not match rpn.num_input_filters")
        self.test_cfg, self.class_names = self.inner.test_cfg, self.inner.class_names

    def children(self):
        return [self.reader, self.inner]

    @property
    def neck(self):
        return self.inner.neck

    @property
    def bbox_head(self):
        return self.inner.bbox_head

    def front_end(self, points, offsets):
        """points [N, 4] f32, offsets [B + 1] i32 -> (canvas [B, H, W, 64] bf16, anchors mask [B, N_anchors] u8, md_voxelize's outputs)"""
        vox = det_ops.voxelize(points, offsets, self.voxel_size, self.pc_range, self.max_points, self.max_voxels)
        voxels, coors, num_points, voxel_num = vox
        canvas = det_ops.pp_pillar_encode(voxels, num_points, coors, voxel_num, self.reader.packed, self.grid_hw, self.reader.voxel_size,
                                          self.reader.offsets)
        mask = det_ops.anchors_mask_batched(coors, voxel_num, (self.grid_hw[1], self.grid_hw[0]), self.inner.anchors_bv, self.voxel_size,
                                            self.pc_range, self.inner.anchor_area_threshold)
        return canvas, mask, vox

    def forward(self, points, offsets, return_aux=False):
        """points [N, 4] f32: the B samples' points back to back; offsets [B + 1] i32 (device) -> (dets [B, nms_post_max_size, 9] f32,
        count [B] i32) as PointPillarsNet.forward.  With test_cfg.streams > 1 the front end runs once for the batch and the inner
        model's forward_streams takes the canvas and the mask."""
        if points.dim() != 2 or points.shape[1] != self.reader.num_input_features:
            raise ValueError(f"PointPillarsKITTIPoints: the reader takes [N, {self.reader.num_input_features}] points, got "
                             f"{tuple(points.shape)}")
        canvas, mask, (voxels, coors, num_points, voxel_num) = self.front_end(points, offsets)
        if return_aux:
            out, aux = self.inner.forward(canvas, mask, return_aux=True)
            return out, dict(aux, voxels=voxels, coors=coors, num_points=num_points, voxel_num=voxel_num, pseudo_image=canvas,
                             anchors_mask=mask)
        if self.inner.streams > 1:
            return self.inner.forward_streams(canvas, mask)
        return self.inner.forward(canvas, mask)

    __call__ = forward

    def loss(self, points, offsets, example, grad=False):
        """the voxeliser and the pillar encoder of forward() (the anchor mask belongs to the targets, not to the loss), then
        PointPillarsNet.loss on the canvas (example: labels, reg_targets of the model's anchors)"""
        voxels, coors, num_points, voxel_num = det_ops.voxelize(points, offsets, self.voxel_size, self.pc_range, self.max_points, self.max_voxels)
        canvas = det_ops.pp_pillar_encode(voxels, num_points, coors, voxel_num, self.reader.packed, self.grid_hw, self.reader.voxel_size,
                                          self.reader.offsets)
        return self.inner.loss(canvas, example, grad=grad)

    def augment_op(self):
        """det_ops.PointCloudAugment with train_cfg["augment"] (None: the reference's defaults) on this model's range"""
        r = self.pc_range
        return self._lazy("augment", lambda: det_ops.PointCloudAugment((r[0], r[1], r[3], r[4]),
                                                                       **dict((self.inner.train_cfg or {}).get("augment") or {})))

    def train_example(self, points, offsets, gt_boxes, gt_classes, gt_count, generator=None, draws=None, valid=None, sampled=None):
        """Raw points and ground truth -> the `example` of loss(), on the device with nothing read back: the training branch of
        prep_pointcloud (det_ops.PointCloudAugment: points [N,4] f32, offsets [B+1] i32, gt_boxes [B,G,7] f32, gt_classes [B,G],
        gt_count [B]; draws = the dict of its draw(), None: drawn with `generator`), the front end on the augmented points, and one
        det_ops.assign_targets per sample on the fixed-capacity box list: the rows from the sample's count on are replaced by a box
        far outside every anchor with class 1, the reference's "ground truth nothing overlaps" case, which changes no target.
        -> dict(labels [B,A] i32, reg_targets [B,A,7] f32, reg_weights [B,A] f32, gt_ids [B,A] i32, anchors_mask [B,A] u8, canvas,
        augment = the dict of PointCloudAugment)."""
        a = self.augment_op()(points, offsets, gt_boxes, gt_classes, gt_count, valid=valid, sampled=sampled, draws=draws, generator=generator)
        canvas, mask, _ = self.front_end(a["points"], a["offsets"])
        boxes, classes = a["gt_boxes"], a["gt_classes"]
        dev, (B, G) = boxes.device, boxes.shape[:2]
        pad = torch.arange(G, device=dev)[None, :] >= a["gt_count"][:, None]
        far = torch.tensor([1e6, 1e6, 0.0, 1.0, 1.0, 1.0, 0.0], dtype=torch.float32, device=dev)
        boxes = torch.where(pad[..., None], far, boxes)
        classes = torch.where(pad, torch.ones_like(classes), classes)
        def thresholds():
            gen = det_ops.generate_anchors(self.inner.generators, (1,) + tuple(self.inner.feature_hw), device=dev)
            return gen["matched_thresholds"].reshape(-1).contiguous(), gen["unmatched_thresholds"].reshape(-1).contiguous()
        mt, ut = self._lazy("thresholds", thresholds)
        rows = [det_ops.assign_targets(self.inner.anchors, boxes[b], classes[b], mt, ut, mask[b]) for b in range(B)]
        labels, reg_targets, reg_weights, gt_ids = (torch.stack([r[i] for r in rows]) for i in range(4))
        return dict(labels=labels, reg_targets=reg_targets, reg_weights=reg_weights, gt_ids=gt_ids, anchors_mask=mask, canvas=canvas, augment=a)

    def train_loss(self, points, offsets, gt_boxes, gt_classes, gt_count, generator=None, draws=None, valid=None, sampled=None, grad=False):
        """train_example, then PointPillarsNet.loss on its canvas: raw points + ground truth -> loss (and, grad=True, d total / d head)
        as one device chain.  -> the dict of loss() plus `example`."""
        ex = self.train_example(points, offsets, gt_boxes, gt_classes, gt_count, generator=generator, draws=draws, valid=valid, sampled=sampled)
        return dict(self.inner.loss(ex["canvas"], ex, grad=grad), example=ex)

    def head_trainer(self, optimizer_cfg=None):
        """PointPillarsNet.head_trainer of the inner model"""
        return self.inner.head_trainer(optimizer_cfg)

    def train_step(self, points, offsets, gt_boxes, gt_classes, gt_count, lr, beta1=0.9, generator=None, draws=None, valid=None, sampled=None):
        """train_example, then HeadTrainer.train_step on its canvas: raw points + ground truth -> one update of the head, as one device
        chain.  -> the dict of HeadTrainer.train_step plus `example`."""
        ex = self.train_example(points, offsets, gt_boxes, gt_classes, gt_count, generator=generator, draws=draws, valid=valid, sampled=sampled)
        return dict(self.head_trainer().train_step(ex["canvas"], ex, lr, beta1), example=ex)

    def _kitti_options(self):
        """test_cfg's KITTI keys: remove_outside_points (True), lidar_input (False), post_center_limit_range (None); the options that
        are not built raise (det_ops.kitti_io_options)"""
        tc = self.test_cfg
        det_ops.kitti_io_options(**{k: tc[k] for k in ("remove_environment", "random_crop", "use_self_train", "fp32_calibration") if k in tc})
        return bool(tc.get("remove_outside_points", True)), bool(tc.get("lidar_input", False)), tc.get("post_center_limit_range")

    def prepare_kitti(self, points, offsets, calib, gt_boxes_camera=None, gt_count=None, reference_detections=None):
        """The camera-frame part of prep_pointcloud (pointpillars/src/data/preprocess.py:59-71, 87) on the device: a raw velodyne scan
        [N,4] f32 with offsets [B+1] and its det_ops.KittiCalibration -> (points, offsets) cut to the camera's view, ready for forward /
        train_example, and -- with gt_boxes_camera [B,G,7] f32 (x, y, z, l, h, w, r) and gt_count [B] -- the lidar ground truth
        [B,G,7] (else None).  Order as the reference's: the frustums of reference_detections (= (bboxes [B,K,4], count [B] or None))
        first, then the image frustum (test_cfg.remove_outside_points, skipped with lidar_input).  Nothing is read back."""
        crop_image, lidar_input, _ = self._kitti_options()
        if points.dim() != 2 or points.shape[1] != 4:
            raise ValueError(f"PointPillarsKITTIPoints: the KITTI crop takes [N, 4] points, got {tuple(points.shape)}")
        if reference_detections is not None:
            bboxes, count = reference_detections if isinstance(reference_detections, (tuple, list)) else (reference_detections, None)
            points, offsets, _ = det_ops.crop_hulls(points, offsets, *calib.detection_frustums(bboxes, count))
        if crop_image and not lidar_input:
            points, offsets, _ = det_ops.crop_hulls(points, offsets, calib.image_frustum(), calib.tensor("image_count"))
        boxes = None
        if gt_boxes_camera is not None:
            if gt_count is None:
                raise ValueError("PointPillarsKITTIPoints: gt_boxes_camera come with gt_count")
            boxes = det_ops.kitti_boxes_to_lidar(gt_boxes_camera, gt_count, calib.tensor("cam2lidar"))
        return points, offsets, boxes

    def forward_kitti(self, points, offsets, calib):
        """A raw velodyne scan and its calibration -> KITTI result rows, as one device chain: prepare_kitti's crop, forward, and
        det_ops.kitti_rows with test_cfg.post_center_limit_range and lidar_input (generate_single_sample_dict_old + predict_kitti_to_anno,
        pointpillars/src/predict.py:204-262, 331-396) -> (rows [B,M,14] f32, src [B,M] i32, out_count [B] i32, dets [B,M,9] f32);
        kitti_eval.rows_to_annos formats them on the host."""
        _, lidar_input, limit = self._kitti_options()
        pts, offs, _ = self.prepare_kitti(points, offsets, calib)
        dets, count = self.forward(pts, offs)
        rows, src, out_count = det_ops.kitti_rows(dets, count, calib.tensor("lidar2cam"), calib.tensor("p2"), calib.tensor("image_shape"),
                                                  limit_range=limit, lidar_input=lidar_input)
        return rows, src, out_count, dets

    def evaluate_kitti(self, rows, count, gt_annos, class_names, current_classes=(0, 1, 2), protocol="full", difficultys=(0, 1, 2)):
        """The official KITTI result of forward_kitti's rows (rows [B,M,14], out_count [B]) against the ground-truth annotation dicts of
        the same B frames, on the device: kitti_eval.PackedEval.with_rows takes the rows as they lie (no host copy), the md_kitti_eval_*
        operators count, kitti_eval.get_official_eval_result(backend="device") divides and prints.  class_names: the detector's label
        names (rows[..., 13] indexes them).  -> what get_official_eval_result returns on rows_to_annos of the same rows."""
        from . import kitti_eval

        table = kitti_eval.CLASS_NAMES_MS if protocol == "ms" else kitti_eval.CLASS_NAMES_FULL
        packed = kitti_eval.pack_annos(gt_annos, None, table, device=rows.device).with_rows(rows, count, class_names)
        return kitti_eval.get_official_eval_result(gt_annos, None, list(current_classes), protocol, difficultys, backend="device", packed=packed)


# ----------------------------------------------------------------------------- YOLOv5 (build-authored; parity unpinned)
SPPF_FUSED = os.environ.get("MD_SPPF_FUSED", "1") != "0"    # A/B knob: 0 = three md_maxpool2d launches + four concat copies per SPPF block
C3_PAIR_FUSED = os.environ.get("MD_C3_PAIR", "1") != "0"   # A/B knob (tools/ab_env_bench.sh): 0 = two md_conv2d launches per C3 bottleneck


def _yconv(init, cin, cout, k=1, s=1, p=None):
    return ConvModule(init, cin, cout, k, s, k // 2 if p is None else p, bn=True, bn_eps=1e-3, act="silu")


class C3(Module):
    """CSP bottleneck with 3 convs: cv3(concat(m(cv1(x)), cv2(x))), m = n x [x (+) cv2_3x3(cv1_1x1(x))]."""

    def __init__(self, init, c1, c2, n=1, shortcut=True):
        c_ = c2 // 2
        self.cv1, self.cv2, self.cv3 = _yconv(init, c1, c_), _yconv(init, c1, c_), _yconv(init, 2 * c_, c2)
        self.m = [(_yconv(init, c_, c_, 1), _yconv(init, c_, c_, 3)) for _ in range(n)]
        self.shortcut, self.c_ = shortcut, c_

    def children(self):
        return [self.cv1, self.cv2, self.cv3] + [m for pair in self.m for m in pair]

    def _derive(self, device):
        self._cv12 = merged_conv([self.cv1, self.cv2], device)
        pk = [nn_ops.pack_c3_pair(a.packed, b.packed) for a, b in self.m]
        self._pairs = pk if all(p is not None for p in pk) else None   # md_c3_pair packs of self.m (None: this width is not fused)

    def __call__(self, x, x_c_off=None, out=None, c_off=0):
        """No copies: one launch computes [cv1(x) | cv2(x)] into the concat buffer; every bottleneck then updates channels [0, c_).
        With 32, 64 or 128 channels a bottleneck is ONE md_c3_pair launch (its 1x1 output stays in LDS; bit-identical; weights as
        md_conv2d packs them: w1[C, roundup(C, 64)], w2[C, roundup(9 C, 64)], korder 0 for C = 32, korder 1 for C = 64 (where the two coincide) and 128): it cannot run in
        place (a tile's halo pixels are other tiles' outputs), so the blocks alternate between two concat buffers and the last one
        carries the cv2(x) half along when it ends in the second.  Other widths: two launches per bottleneck, in place (the 1x1 reads the
        slice, the 3x3 adds the slice as residual and writes it back: each element is read and written by the same thread)."""
        cat = nn_ops.conv2d(x, self._cv12, x_c_off=x_c_off)
        if C3_PAIR_FUSED and self._pairs is not None:
            bufs = (cat, torch.empty_like(cat))   # block i reads bufs[i % 2], writes bufs[(i + 1) % 2]; cv2(x) sits in bufs[0]
            npairs = len(self._pairs)
            for i, pk in enumerate(self._pairs):
                # an odd chain ends in bufs[1]: its last block (which reads bufs[0]) carries the cv2(x) half along -- cv3 reads one buffer
                nn_ops.c3_pair(bufs[i % 2], pk, bufs[(i + 1) % 2], 0, 0, self.shortcut, pass_through=(i + 1 == npairs and npairs % 2 == 1))
            return self.cv3(bufs[npairs % 2], out=out, c_off=c_off)
        for a, b in self.m:
            t = a(cat, x_c_off=0)
            if self.shortcut:
                b(t, residual=cat, res_c_off=0, out=cat, c_off=0)     # SiLU first, then the shortcut add (md_conv2d relu code 2)
            else:
                b(t, out=cat, c_off=0)
        return self.cv3(cat, out=out, c_off=c_off)


class SPPF(Module):
    def __init__(self, init, c1, c2, k=5):
        c_ = c1 // 2
        self.cv1, self.cv2, self.k, self.c_ = _yconv(init, c1, c_), _yconv(init, 4 * c_, c2), k, c_

    def children(self):
        return [self.cv1, self.cv2]

    def __call__(self, x, out=None, c_off=0):
        n, h, w, _ = x.shape
        cat = torch.empty((n, h, w, 4 * self.c_), dtype=torch.bfloat16, device=x.device)
        if SPPF_FUSED and nn_ops.sppf_pool_fits(h, w, self.c_):
            # cv1 writes the first slice of the concat buffer; ONE launch fills the other three (md_sppf_pool; equal as numbers, a zero maximum may differ in sign)
            self.cv1(x, out=cat, c_off=0)
            nn_ops.sppf_pool(cat, self.c_, self.k)
            return self.cv2(cat, out=out, c_off=c_off)
        y = self.cv1(x)
        nn_ops.concat_copy(y, cat, 0)
        for i in range(1, 4):
            y = nn_ops.maxpool2d(y, self.k, 1, self.k // 2, zero_pad=False)
            nn_ops.concat_copy(y, cat, i * self.c_)
        return self.cv2(cat, out=out, c_off=c_off)


class _YOLO(Module):
    """What YOLOv5 and YOLOv8 share: the stem conv `b0` with its stem-layout form, and everything behind the decode."""

    def _derive(self, device):
        # the 3-channel stride-2 stem conv on the 4-channel stem layout (md_stem_conv) when the batch arrives in it
        self.stem = nn_ops.pack_stem_conv(self.b0.weight, bn=self.b0.bn, bias=self.b0.bias, act=self.b0.act)
        if self.stem is not None:
            self.stem.to(device)

    def _stem(self, x):
        """x: [N,H,W,8] bf16 NHWC (3 real channels), or the batch in the stem layout ([N,H+16,W+16,4], nn_ops.to_stem_layout)."""
        if x.shape[3] != 4:
            return self.b0(x)
        if self.stem is None:
            raise nn_ops._lib.MindDetHipError("stem-layout input needs a 6x6 / 3x3 stride-2 stem conv with 32 or 64 output channels")
        return nn_ops.stem_conv(x, self.stem)

    def _detections(self, heads, boxes, scores, labels, return_aux):
        """decoded candidates [B, total, ...] -> per image the top nms_pre, class-aware NMS, (dets [B,max_det,6], count [B])"""
        B, total = scores.shape
        seg = self.const((B, total), lambda: _segments(B, total, scores.device))
        sv, si, sc = det_ops.topk_segmented(scores, seg, self.nms_pre, max_segment=total)
        sb = det_ops.gather_rows(boxes, si, sc)
        sl = torch.gather(labels, 1, si.long())
        keep, kidx, num = det_ops.nms_aligned(sb, self.iou_thres, mode=det_ops.NMS_MODE_STRICT, count=sc, group=sl,
                                              max_output=self.max_det)
        dets, count = det_ops.pack_detections(sb, sv, sl, kidx, num, self.max_det, sel_cnt=sc,
                                              status=self.prefix_status.tensor(B, scores.device))
        if return_aux:
            return dets, count, dict(heads=heads, boxes=boxes, scores=scores, labels=labels, sel_idx=si, sel_cnt=sc,
                                     sel_boxes=sb, sel_labels=sl, keep=keep)
        return dets, count


@DETECTORS.register_module
class YOLOv5(_YOLO):
    """YOLOv5 (Ultralytics v6/v7 layout): CSPDarknet backbone + PANet head + Detect, single-label decode and
    class-aware NMS (conf 0.25 / IoU 0.45 / max_det 300 by default).  depth_multiple/width_multiple 0.33/0.5 = yolov5s."""
    ANCHORS = ((10, 13, 16, 30, 33, 23), (30, 61, 62, 45, 59, 119), (116, 90, 156, 198, 373, 326))

    def __init__(self, depth_multiple=0.33, width_multiple=0.5, num_classes=80, conf_thres=0.25, iou_thres=0.45,
                 max_det=300, nms_pre=4096, seed=7, train_cfg=None, test_cfg=None):
        init = ParamInit(seed)
        _split_forward_of(self, test_cfg)
        ch = lambda c: max(8, int(math.ceil(c * width_multiple / 8) * 8))
        d = lambda n: max(1, round(n * depth_multiple))
        c64, c128, c256, c512, c1024 = ch(64), ch(128), ch(256), ch(512), ch(1024)
        self.b0 = _yconv(init, 3, c64, 6, 2, 2)
        self.b1 = _yconv(init, c64, c128, 3, 2)
        self.b2 = C3(init, c128, c128, d(3))
        self.b3 = _yconv(init, c128, c256, 3, 2)
        self.b4 = C3(init, c256, c256, d(6))
        self.b5 = _yconv(init, c256, c512, 3, 2)
        self.b6 = C3(init, c512, c512, d(9))
        self.b7 = _yconv(init, c512, c1024, 3, 2)
        self.b8 = C3(init, c1024, c1024, d(3))
        self.b9 = SPPF(init, c1024, c1024)
        self.h10 = _yconv(init, c1024, c512, 1)
        self.h13 = C3(init, 2 * c512, c512, d(3), False)
        self.h14 = _yconv(init, c512, c256, 1)
        self.h17 = C3(init, 2 * c256, c256, d(3), False)
        self.h18 = _yconv(init, c256, c256, 3, 2)
        self.h20 = C3(init, 2 * c256, c512, d(3), False)
        self.h21 = _yconv(init, c512, c512, 3, 2)
        self.h23 = C3(init, 2 * c512, c1024, d(3), False)
        self.nc, self.na = num_classes, 3
        no = self.na * (5 + num_classes)
        self.detect = [ConvModule(init, c, no, 1, bn=False, relu=False, bias=True, std=0.02) for c in (c256, c512, c1024)]
        self.strides = (8, 16, 32)
        self.conf_thres, self.iou_thres, self.max_det, self.nms_pre = conf_thres, iou_thres, max_det, nms_pre
        self.prefix_status = det_ops.PrefixStatus()   # sticky flags of the top-nms_pre cut (see StandardRoIHead)
        self.c = (c256, c512)

    def children(self):
        return ([self.b0, self.b1, self.b3, self.b5, self.b7, self.h10, self.h14, self.h18, self.h21] + self.detect +
                [self.b2, self.b4, self.b6, self.b8, self.b9, self.h13, self.h17, self.h20, self.h23])

    def features(self, x):
        """x: see _stem"""
        x = self.b3(self.b2(self.b1(self._stem(x))))
        # p3 / p4 are produced straight into the second half of the PAN concat buffers that consume them later
        # ([upsampled top | skip]); the next backbone conv reads them as a channel slice
        n, h, w, _ = x.shape
        c = self.b4.cv3.cout
        cat17 = torch.empty((n, h, w, 2 * c), dtype=torch.bfloat16, device=x.device)
        self.b4(x, out=cat17, c_off=c)
        x = self.b5(cat17, x_c_off=c)
        n, h, w, _ = x.shape
        c = self.b6.cv3.cout
        cat13 = torch.empty((n, h, w, 2 * c), dtype=torch.bfloat16, device=x.device)
        self.b6(x, out=cat13, c_off=c)
        x = self.b9(self.b8(self.b7(cat13, x_c_off=c)))
        # h10 / h14 are written straight into the second half of the bottom-up concat buffers that consume them later ([downsampled | top]);
        # the top-down upsample reads them there as a channel slice (r04: two concat copies less)
        n, h, w, _ = x.shape
        c = self.h10.cout
        cat23 = torch.empty((n, h, w, 2 * c), dtype=torch.bfloat16, device=x.device)
        self.h10(x, out=cat23, c_off=c)
        nn_ops.upsample2x(cat23, cat13, 0, src_c0=c, width=c)
        n, h, w, _ = cat13.shape
        c = self.h14.cout
        cat20 = torch.empty((n, h, w, 2 * c), dtype=torch.bfloat16, device=x.device)
        self.h14(self.h13(cat13), out=cat20, c_off=c)
        nn_ops.upsample2x(cat20, cat17, 0, src_c0=c, width=c)
        o3 = self.h17(cat17)
        self.h18(o3, out=cat20, c_off=0)
        o4 = self.h20(cat20)
        self.h21(o4, out=cat23, c_off=0)
        o5 = self.h23(cat23)
        return [d(o) for d, o in zip(self.detect, (o3, o4, o5))]

    def forward(self, images, return_aux=False):
        heads = self.features(images)
        B = images.shape[0]
        dev = images.device
        total = sum(h.shape[1] * h.shape[2] * self.na for h in heads)
        boxes = torch.empty((B, total, 4), dtype=torch.float32, device=dev)
        scores = torch.empty((B, total), dtype=torch.float32, device=dev)
        labels = torch.empty((B, total), dtype=torch.int32, device=dev)
        off = 0
        for h, s, anc in zip(heads, self.strides, self.ANCHORS):
            det_ops.yolo_decode(h, boxes, scores, labels, self.nc, self.na, s, anc, self.conf_thres, off, total)
            off += h.shape[1] * h.shape[2] * self.na
        return self._detections(heads, boxes, scores, labels, return_aux)

    __call__ = forward


# ----------------------------------------------------------------------------- YOLOv8 (BASELINE configs[3]; parity unpinned)
class C2f(Module):
    """Ultralytics C2f: cv2(concat(y0, y1, m1(y1), m2(m1(y1)), ...)) with (y0, y1) = chunk(cv1(x), 2) and m = n x
    [x (+) 3x3(3x3(x))].  cv1 is stored as its two output halves (cv1a, cv1b: the same arithmetic as one 2c-channel 1x1
    conv followed by chunk), so that y0 is written straight into the concat buffer and y1 is a compact tensor."""

    def __init__(self, init, c1, c2, n=1, shortcut=False):
        c = c2 // 2
        self.c, self.n, self.shortcut = c, n, shortcut
        self.cv1a, self.cv1b = _yconv(init, c1, c, 1), _yconv(init, c1, c, 1)
        self.cv2 = _yconv(init, (2 + n) * c, c2, 1)
        self.m = [(_yconv(init, c, c, 3), _yconv(init, c, c, 3)) for _ in range(n)]

    def children(self):
        return [self.cv1a, self.cv1b, self.cv2] + [m for pair in self.m for m in pair]

    def _derive(self, device):
        self._cv1 = merged_conv([self.cv1a, self.cv1b], device)

    def __call__(self, x, x_c_off=None, out=None, c_off=0):
        """No copies: one launch writes (y0 | y1) = cv1(x) into channels [0, 2c) of the concat buffer; bottleneck i reads its
        input (and its shortcut) as channels [(1+i)c, (2+i)c) of that buffer and writes [(2+i)c, (3+i)c)."""
        n, h, w, _ = x.shape
        c = self.c
        cat = torch.empty((n, h, w, (2 + self.n) * c), dtype=torch.bfloat16, device=x.device)
        nn_ops.conv2d(x, self._cv1, out=cat, c_off=0, x_c_off=x_c_off)
        for i, (a, b) in enumerate(self.m):
            t = a(cat, x_c_off=(1 + i) * c)
            if self.shortcut:
                b(t, residual=cat, res_c_off=(1 + i) * c, out=cat, c_off=(2 + i) * c)   # SiLU first, then the shortcut add
            else:
                b(t, out=cat, c_off=(2 + i) * c)
        return self.cv2(cat, out=out, c_off=c_off)


@DETECTORS.register_module
class YOLOv8(_YOLO):
    """YOLOv8 (Ultralytics v8.0 yolov8.yaml): CSP backbone with C2f blocks + SPPF, PAN head, anchor-free Detect with DFL
    (reg_max 16); decode + class-aware NMS (conf 0.25 / IoU 0.7 / max_det 300).  depth / width / max_channels 1.0 / 1.0 / 512
    = yolov8l."""

    def __init__(self, depth_multiple=1.0, width_multiple=1.0, max_channels=512, num_classes=80, reg_max=16, conf_thres=0.25,
                 iou_thres=0.7, max_det=300, nms_pre=4096, seed=7, train_cfg=None, test_cfg=None):
        init = ParamInit(seed)
        _split_forward_of(self, test_cfg)
        ch = lambda c: max(8, int(math.ceil(min(c, max_channels) * width_multiple / 8) * 8))
        d = lambda n: max(1, round(n * depth_multiple))
        c64, c128, c256, c512, c1024 = ch(64), ch(128), ch(256), ch(512), ch(1024)
        self.b0 = _yconv(init, 3, c64, 3, 2)
        self.b1 = _yconv(init, c64, c128, 3, 2)
        self.b2 = C2f(init, c128, c128, d(3), True)
        self.b3 = _yconv(init, c128, c256, 3, 2)
        self.b4 = C2f(init, c256, c256, d(6), True)
        self.b5 = _yconv(init, c256, c512, 3, 2)
        self.b6 = C2f(init, c512, c512, d(6), True)
        self.b7 = _yconv(init, c512, c1024, 3, 2)
        self.b8 = C2f(init, c1024, c1024, d(3), True)
        self.b9 = SPPF(init, c1024, c1024)
        self.h12 = C2f(init, c1024 + c512, c512, d(3))
        self.h15 = C2f(init, c512 + c256, c256, d(3))
        self.h16 = _yconv(init, c256, c256, 3, 2)
        self.h18 = C2f(init, c256 + c512, c512, d(3))
        self.h19 = _yconv(init, c512, c512, 3, 2)
        self.h21 = C2f(init, c512 + c1024, c1024, d(3))
        self.nc, self.reg_max = num_classes, reg_max
        c2 = max(16, c256 // 4, 4 * reg_max)
        c3 = max(c256, min(num_classes, 100))
        self.head_c = (4 * reg_max + num_classes + 7) // 8 * 8
        self.box, self.cls = [], []
        for c in (c256, c512, c1024):
            self.box.append([_yconv(init, c, c2, 3), _yconv(init, c2, c2, 3),
                             ConvModule(init, c2, 4 * reg_max, 1, bn=False, relu=False, bias=True, std=0.05, bias_value=1.0)])
            self.cls.append([_yconv(init, c, c3, 3), _yconv(init, c3, c3, 3),
                             ConvModule(init, c3, num_classes, 1, bn=False, relu=False, bias=True, std=0.05)])
        self.strides = (8, 16, 32)
        self.conf_thres, self.iou_thres, self.max_det, self.nms_pre = conf_thres, iou_thres, max_det, nms_pre
        self.prefix_status = det_ops.PrefixStatus()   # sticky flags of the top-nms_pre cut (see StandardRoIHead)

    def children(self):
        return ([self.b0, self.b1, self.b3, self.b5, self.b7, self.h16, self.h19] +
                [self.b2, self.b4, self.b6, self.b8, self.b9, self.h12, self.h15, self.h18, self.h21] +
                [m for br in self.box + self.cls for m in br])

    def _derive(self, device):
        super()._derive(device)
        self._stem2 = [merged_conv([bx[0], cl[0]], device) for bx, cl in zip(self.box, self.cls)]   # a level's two branch stems read f once

    def features(self, x):
        """x: see _stem"""
        x = self.b3(self.b2(self.b1(self._stem(x))))
        # p3 / p4 are produced straight into the PAN concat buffers that consume them later ([upsampled top | skip]); the next
        # backbone conv reads them as a channel slice
        n, h, w, _ = x.shape
        c_top = self.h12.cv2.cout
        cat15 = torch.empty((n, h, w, c_top + self.b4.cv2.cout), dtype=torch.bfloat16, device=x.device)
        self.b4(x, out=cat15, c_off=c_top)
        x = self.b5(cat15, x_c_off=c_top)
        n, h, w, _ = x.shape
        c_top = self.b9.cv2.cout
        cat12 = torch.empty((n, h, w, c_top + self.b6.cv2.cout), dtype=torch.bfloat16, device=x.device)
        self.b6(x, out=cat12, c_off=c_top)
        # p5 / h12 are written straight into the second part of the bottom-up concat buffers that consume them later ([downsampled | top]);
        # the top-down upsample reads them there as a channel slice (r04: two concat copies less)
        x = self.b8(self.b7(cat12, x_c_off=c_top))
        n, h, w, _ = x.shape
        c19, c5 = self.h19.cout, self.b9.cv2.cout
        cat21 = torch.empty((n, h, w, c19 + c5), dtype=torch.bfloat16, device=x.device)
        self.b9(x, out=cat21, c_off=c19)
        nn_ops.upsample2x(cat21, cat12, 0, src_c0=c19, width=c5)
        n, h, w, _ = cat12.shape
        c16, c12 = self.h16.cout, self.h12.cv2.cout
        cat18 = torch.empty((n, h, w, c16 + c12), dtype=torch.bfloat16, device=x.device)
        self.h12(cat12, out=cat18, c_off=c16)
        nn_ops.upsample2x(cat18, cat15, 0, src_c0=c16, width=c12)
        o3 = self.h15(cat15)
        self.h16(o3, out=cat18, c_off=0)
        o4 = self.h18(cat18)
        self.h19(o4, out=cat21, c_off=0)
        o5 = self.h21(cat21)
        heads = []
        for f, bx, cl, stem2 in zip((o3, o4, o5), self.box, self.cls, self._stem2):
            n, h, w, _ = f.shape
            # (the two branch convs write every channel unless the class count needed padding to a multiple of 8: only then a zero fill)
            full = self.head_c == 4 * self.reg_max + cl[2].cout
            head = (torch.empty if full else torch.zeros)((n, h, w, self.head_c), dtype=torch.bfloat16, device=f.device)
            t = nn_ops.conv2d(f, stem2)                                     # the two branch stems: one launch
            bx[2](bx[1](t, x_c_off=0), out=head, c_off=0)                   # 4 * reg_max distribution logits
            cl[2](cl[1](t, x_c_off=bx[0].cout), out=head, c_off=4 * self.reg_max)   # class logits
            heads.append(head)
        return heads

    def forward(self, images, return_aux=False):
        heads = self.features(images)
        B, dev = images.shape[0], images.device
        total = sum(h.shape[1] * h.shape[2] for h in heads)
        boxes = torch.empty((B, total, 4), dtype=torch.float32, device=dev)
        scores = torch.empty((B, total), dtype=torch.float32, device=dev)
        labels = torch.empty((B, total), dtype=torch.int32, device=dev)
        off = 0
        for h, s in zip(heads, self.strides):
            det_ops.yolov8_decode(h, boxes, scores, labels, self.nc, self.reg_max, s, self.conf_thres, off, total)
            off += h.shape[1] * h.shape[2]
        return self._detections(heads, boxes, scores, labels, return_aux)

    __call__ = forward

