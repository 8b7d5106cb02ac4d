"""graphs.Module: `.to()` on a sub-module alone repacks its convs, rebuilds the packs derived from them, empties its device constants
and advances the pack generation graphs.SplitForward keys its priming pass on.  All packing is torch on the CPU."""
import torch

from minddet_amd import graphs, nn_ops


def _pack_tensors(pk):
    return {k: v for k, v in vars(pk).items() if isinstance(v, torch.Tensor)}


def _same(a, b):
    ta, tb = _pack_tensors(a), _pack_tensors(b)
    return ta.keys() == tb.keys() and len(ta) > 0 and all(torch.equal(ta[k], tb[k]) for k in ta)


def _new_weights(mod):
    for m in mod.modules():
        m.weight = m.weight * 0.5 + 0.01


def test_modules_are_the_leaves_in_children_order():
    bb = graphs.ResNet(depth=50, layers=[1, 1, 1, 1])
    b0 = bb.stages[0][0]
    assert b0.modules() == [b0.conv1, b0.conv2, b0.conv3, b0.downsample]
    assert bb.modules() == [bb.conv1] + [m for st in bb.stages for b in st for m in b.modules()]
    assert bb.conv1.modules() == [bb.conv1] and bb.conv_modules() == bb.modules()


def test_submodule_to_rebuilds_derived_packs_and_advances_the_generation():
    bb = graphs.ResNet(depth=50, layers=[1, 1, 1, 1]).to("cpu")
    first, later = bb.stages[0][0], bb.stages[1][0]
    assert first._fused is not None and later._fused is None and later._dual is not None and bb.stem is not None
    old = (first._fused, later._dual, bb.stem)
    bb.const("k", lambda: torch.zeros(1))
    gen0 = graphs.Module.generation
    _new_weights(bb)
    assert graphs.Module.generation == gen0            # only .to() makes packs
    bb.to("cpu")
    assert graphs.Module.generation != gen0 and bb._consts == {}
    ds = first.downsample.packed
    want = nn_ops.pack_bottleneck(nn_ops.pack_conv(first.conv1.weight, bn=first.conv1.bn, relu=True),
                                  nn_ops.pack_conv(first.conv2.weight, bn=first.conv2.bn, stride=1, pad=1, relu=True),
                                  nn_ops.pack_conv(first.conv3.weight, bn=first.conv3.bn, relu=True), ds)
    assert _same(first._fused, want) and not _same(first._fused, old[0])
    assert _same(later._dual, nn_ops.pack_dual(later.conv3.packed, later.downsample.packed)) and not _same(later._dual, old[1])
    assert _same(bb.stem, nn_ops.pack_stem(bb.conv1.weight, bn=bb.conv1.bn)) and not _same(bb.stem, old[2])


def test_backbone_to_inside_a_detector_advances_the_generation_split_forward_reads():
    """model.backbone.to(dev) after a backbone reload: new fused / dual packs, so SplitForward must prime again"""
    from minddet.models import Config, build_detector

    cfg = Config.fromfile("configs/faster_rcnn/faster_rcnn_tiny.py")
    m = build_detector(cfg.model, cfg.train_cfg, cfg.test_cfg).to("cpu")
    m.rpn_head.const("k", lambda: torch.zeros(1))
    gen0 = graphs.Module.generation
    m.backbone.to("cpu")
    assert graphs.Module.generation != gen0
    assert "k" in m.rpn_head._consts                  # another part's constants stay
    m.to("cpu")
    assert m.rpn_head._consts == {}


def test_c3_to_rebuilds_merged_and_pair_packs_whatever_the_knob():
    blk = graphs.C3(graphs.ParamInit(3), 128, 128, 2).to("cpu")
    assert blk._pairs is not None and len(blk._pairs) == 2
    old_cv12, old_pairs = blk._cv12, blk._pairs
    knob = graphs.C3_PAIR_FUSED
    graphs.C3_PAIR_FUSED = False                          # the knob selects a path at call time; it is not a pack state
    try:
        _new_weights(blk)
        blk.to("cpu")
    finally:
        graphs.C3_PAIR_FUSED = knob
    assert _same(blk._cv12, graphs.merged_conv([blk.cv1, blk.cv2], "cpu")) and not _same(blk._cv12, old_cv12)
    for pk, was, (a, b) in zip(blk._pairs, old_pairs, blk.m):
        assert _same(pk, nn_ops.pack_c3_pair(a.packed, b.packed)) and not _same(pk, was)
    wide = graphs.C3(graphs.ParamInit(3), 512, 512, 1).to("cpu")
    assert wide._pairs is None                            # 256 channels: md_c3_pair does not take the width
