"""GPU: the CenterNet training input (include/minddet_hip_cnaug.h) through the C ABI and through graphs.CenterNet.

md_cn_aug_transform: all three outputs bit-equal to tests/cnaug_contract.py.  md_cn_aug_image without colour: bit-equal to
md_image_preprocess; with colour: the border and the spare channels exactly +0 in an output pre-filled with 0xFF, every other element
equal to the contract's bf16 except at most 1 in 10^4 that differ by 1 bf16 ulp (the contract's gs_mean is exactly rounded, the
device's is a fixed-order float64 sum: tests/test_cn_augment_cpu.py bounds what that can move).  Then determinism and the call forms,
the flip folded into the matrix, the chain into the targets and the loss on the tiny config, the draws, and the ABI rows."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import cnaug_contract as cc
from tests.conftest import has_gpu
from tests.test_cn_augment_cpu import attrs_of, fixture

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.40789654, 0.44719302, 0.47026115), (0.28863828, 0.27408164, 0.27809835)
ATTRS = dict(scale=0.4, shift=0.1, flip_prop=0.5)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared problems are read-only arrays)


def bits16(t):
    torch.cuda.synchronize()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def check_transform(tag, sizes, draws, **kw):
    from minddet_amd import det_ops

    want = cc.transform(sizes, draws, **kw)
    mat_in, trans_out, flip_width = det_ops.cn_aug_transform(dev(sizes.astype(np.int32)), dev(draws), **kw)
    torch.cuda.synchronize()
    got = dict(mat_in=mat_in.cpu().numpy(), trans_out=trans_out.cpu().numpy(), flip_width=flip_width.cpu().numpy())
    bad = {k: int((got[k].view(np.int32 if got[k].itemsize == 4 else np.int64) != want[k].view(np.int32 if want[k].itemsize == 4 else np.int64)).sum())
           for k in got}
    print(f"cn_aug_transform[{tag}]: elements that differ from the contract {bad}, flipped {int(want['flipped'].sum())} of {len(sizes)}")
    assert all(got[k].dtype == want[k].dtype and got[k].shape == want[k].shape for k in got) and not any(bad.values()), bad
    return want


def test_transform_equals_the_contract_on_the_fixture():
    f = fixture()
    for mode in (True, False):
        idx = np.flatnonzero(f["rand_crop"] == mode)
        check_transform(f"fixture, rand_crop {mode}", f["size"][idx], f["draws"][idx], **attrs_of(f, int(idx[0])))


@pytest.mark.parametrize("rand_crop", [True, False])
def test_transform_equals_the_contract_on_a_seeded_batch(rand_crop):
    """67 samples (two workgroups of 64 lanes): sizes from 1 x 1 to 700 x 900, flipped and not, a draw that puts c outside the image, both
    ends of flip_prop, a size below 1"""
    rng = np.random.default_rng(67 + rand_crop)
    B = 67
    sizes = np.stack([rng.integers(1, 701, B), rng.integers(1, 901, B)], 1)
    sizes[0], sizes[1], sizes[2], sizes[66] = (1, 1), (700, 900), (1, 900), (37, 53)
    draws = np.zeros((B, 4))
    if rand_crop:
        draws[:, 0] = np.arange(0.6, 1.4, 0.1)[rng.integers(0, 8, B)]
        draws[:, 1] = np.floor(rng.uniform(0, 1, B) * sizes[:, 1])
        draws[:, 2] = np.floor(rng.uniform(0, 1, B) * sizes[:, 0])
        draws[3, 1:3], draws[4, 1:3] = (-50.0, 2000.0), (5000.0, -3.0)               # c outside the image
    else:
        draws[:, :3] = rng.normal(size=(B, 3))
        draws[3, :3], draws[4, :3] = (25.0, -25.0, 9.0), (-2.0, 2.0, -1.0)           # clipped far out, and on the clips' edges
    draws[:, 3] = rng.uniform(0, 1, B)
    draws[5, 3], draws[6, 3] = 0.5, np.nextafter(0.5, 0)                             # not flipped / flipped at the threshold
    want = check_transform("seeded", sizes, draws, rand_crop=rand_crop, input_hw=(96, 160), down_ratio=4, **ATTRS)
    assert not want["flipped"][5] and want["flipped"][6] and 10 <= want["flipped"].sum() <= 57      # both branches, many times
    assert not rand_crop or (want["c"][3] < 0).any() or (want["c"][3] > sizes[3][::-1]).any()
    never = check_transform("flip_prop 0", sizes, draws, rand_crop=rand_crop, input_hw=(512, 512), down_ratio=4, scale=0.4, shift=0.1, flip_prop=0.0)
    always = check_transform("flip_prop 1", sizes, draws, rand_crop=rand_crop, input_hw=(64, 96), down_ratio=2, scale=0.0, shift=0.0, flip_prop=1.0)
    assert not never["flipped"].any() and always["flipped"].all() and np.array_equal(always["flip_width"], sizes[:, 1])
    sizes[7], sizes[8] = (0, 40), (30, -2)                                            # an error only the device can see: zeros
    zero = check_transform("sizes below 1", sizes, draws, rand_crop=rand_crop, input_hw=(96, 160), down_ratio=4, **ATTRS)
    assert not zero["mat_in"][7:9].any() and not zero["trans_out"][7:9].any() and not zero["flip_width"][7:9].any()


@functools.lru_cache(maxsize=None)
def image_problem(out_hw=(24, 40)):
    """B = 3: sources 37 x 53, 64 x 64 and 5 x 200 padded to 64 x 200 with 255, matrices from the contract's transform (rand_crop, one
    sample flipped), seeded colour draws"""
    rng = np.random.default_rng(out_hw[0])
    sizes = np.array([(37, 53), (64, 64), (5, 200)], np.int32)
    img = np.full((3, 64, 200, 3), 255, np.uint8)
    for b, (h, w) in enumerate(sizes):
        img[b, :h, :w] = rng.integers(0, 256, (h, w, 3))
    draws = np.array([(0.9, 20.0, 17.0, 0.9), (1.2, 40.0, 30.0, 0.1), (0.7, 110.0, 2.0, 0.7)])
    t = cc.transform(sizes, draws, rand_crop=True, input_hw=out_hw, down_ratio=4, **ATTRS)
    assert t["flipped"].tolist() == [False, True, False]
    col = np.zeros((3, 8))
    col[:, :3] = 1.0 + rng.uniform(-0.4, 0.4, (3, 3))
    col[:, 3:6] = rng.normal(0, 0.03, (3, 3))
    for a in (img, sizes, t["mat_in"], col):
        a.setflags(write=False)
    return img, sizes, t["mat_in"], col


def colour_with(col, orders):
    c = np.array(col)
    c[:, 6] = orders
    return c


def run_image(img, sizes, mat, col, out_hw, stem_layout, **kw):
    from minddet_amd import det_ops

    out = det_ops.cn_aug_image(dev(img), dev(sizes), dev(mat), MEAN, STD, out_hw, colour=None if col is None else dev(col), stem_layout=stem_layout, **kw)
    return bits16(out)


def check_colour(tag, got, img, sizes, mat, col, out_hw, stem_layout):
    lo, hi, C = (7, 9, 4) if stem_layout else (0, 0, 8)
    want = cc.image(img, sizes, mat, MEAN, STD, out_hw, col=col, pad=(lo, hi), C=C)
    ho, wo = out_hw
    area = np.zeros(got.shape, bool)
    area[:, lo:lo + ho, lo:lo + wo, :3] = True
    stray = int((got[~area] != 0).sum())                       # the border and the spare channels: +0, bit for bit
    ndiff, worst = cc.bf16_differences(got[area], want[area])
    n = int(area.sum())
    print(f"cn_aug_image[{tag}]: {ndiff} of {n} image elements differ from the contract, worst {worst} bf16 ulp; non-zero outside the image area {stray}")
    assert got.shape == want.shape and stray == 0
    assert worst <= 1 and ndiff * 10000 <= n, (ndiff, worst, n)
    return want


@pytest.mark.parametrize("stem_layout", [True, False], ids=["C4 stem padding", "C8 pad 0"])
def test_without_colour_the_image_equals_image_preprocess_bit_for_bit(stem_layout):
    from minddet_amd import nn_ops

    img, sizes, mat, _ = image_problem()
    full = np.array([(64, 200)] * 3, np.int32)
    got = run_image(img, full, mat, None, (24, 40), stem_layout)
    ref = bits16(nn_ops.image_preprocess(dev(img), dev(mat), MEAN, STD, (24, 40), stem_layout=stem_layout))
    assert np.array_equal(got, ref) and got.any()
    # the samples' own extents: each row equals md_image_preprocess on the cropped sample, and the 255 of the padding reads as border
    got = run_image(img, sizes, mat, None, (24, 40), stem_layout)
    for b, (h, w) in enumerate(sizes):
        crop = np.ascontiguousarray(img[b:b + 1, :h, :w])
        ref = bits16(nn_ops.image_preprocess(dev(crop), dev(mat[b:b + 1]), MEAN, STD, (24, 40), stem_layout=stem_layout))
        assert np.array_equal(got[b:b + 1], ref), b
    lo, hi, C = (7, 9, 4) if stem_layout else (0, 0, 8)
    want = cc.image(img, sizes, mat, MEAN, STD, (24, 40), col=None, pad=(lo, hi), C=C)
    ndiff, worst = cc.bf16_differences(got, want)
    print(f"cn_aug_image[no colour, {C} channels]: {ndiff} of {got.size} elements differ from the contract's restatement, worst {worst} bf16 ulp")
    assert worst <= 1 and ndiff * 10000 <= got.size
    black = cc.bf16_bits(cc.plain(np.zeros((1, 3), np.float32), MEAN, STD))[0]
    assert (got[2, lo + 23, lo:lo + 40, :3] == black).all()          # the 5-row sample: far rows are border, not the 255 below it


@pytest.mark.parametrize("orders", [(0, 1, 2), (3, 4, 5)])
@pytest.mark.parametrize("stem_layout", [True, False], ids=["C4", "C8"])
def test_with_colour_the_image_equals_the_contract(orders, stem_layout):
    from minddet_amd import det_ops

    img, sizes, mat, col = image_problem()
    col = colour_with(col, orders)
    lo, hi, C = (7, 9, 4) if stem_layout else (0, 0, 8)
    out = torch.empty((3, 24 + lo + hi, 40 + lo + hi, C), dtype=torch.bfloat16, device=DEV)
    out.view(torch.uint8).fill_(0xFF)
    det_ops.cn_aug_image(dev(img), dev(sizes), dev(mat), MEAN, STD, (24, 40), colour=dev(col), stem_layout=stem_layout, out=out)
    got = bits16(out)
    check_colour(f"orders {orders}, C = {C}", got, img, sizes, mat, col, (24, 40), stem_layout)
    plain = run_image(img, sizes, mat, None, (24, 40), stem_layout)
    assert (got != plain).sum() > 2000                               # the colour chain did run (2880 image elements)


def test_with_colour_on_an_output_of_several_chunks():
    """70 x 130 = 9100 output pixels per sample: five partial sums (the last one of 908 pixels), 36 workgroups of the output pass per
    sample, the last one partly idle"""
    img, sizes, _, col = image_problem()
    draws = np.array([(1.1, 25.0, 19.0, 0.2), (0.8, 31.0, 33.0, 0.8), (1.3, 90.0, 3.0, 0.3)])
    mat = cc.transform(sizes, draws, rand_crop=True, input_hw=(70, 130), down_ratio=2, **ATTRS)["mat_in"]
    col = colour_with(col, (5, 2, 1))
    for stem_layout in (False, True):
        from minddet_amd import det_ops

        lo, hi, C = (7, 9, 4) if stem_layout else (0, 0, 8)
        out = torch.empty((3, 70 + lo + hi, 130 + lo + hi, C), dtype=torch.bfloat16, device=DEV)
        out.view(torch.uint8).fill_(0xFF)
        det_ops.cn_aug_image(dev(img), dev(sizes), dev(mat), MEAN, STD, (70, 130), colour=dev(col), stem_layout=stem_layout, out=out)
        check_colour(f"70 x 130, C = {C}", bits16(out), img, sizes, mat, col, (70, 130), stem_layout)


def test_positions_outside_the_image_and_non_finite_matrices_give_the_black_level():
    img, sizes, mat, col = image_problem()
    nan, inf = np.nan, np.inf
    mats = np.array([(1, 0, 500, 0, 1, 0), (1, 0, 0, 0, 1, -400), (nan, 0, 3, 0, 1, 2), (1, 0, inf, 0, 1, 2), (1, 0, 3, 0, -inf, 2), (1, nan, 3, nan, 1, 2),
                     (1e30, 0, 0, 0, 1e30, 0), (1, 0, 3, 0, 1, 2)], np.float32)
    B = len(mats)
    imgs = np.ascontiguousarray(np.broadcast_to(img[1], (B,) + img.shape[1:]))
    sz = np.array([(64, 64)] * B, np.int32)
    black = cc.bf16_bits(cc.plain(np.zeros((1, 3), np.float32), MEAN, STD))[0]
    got = run_image(imgs, sz, mats, None, (24, 40), False)
    assert (got[6, 0, 0, :3] != black).any()                         # (1e30 x 0 is 0: the first pixel of that sample is a real one)
    got[6, 0, 0, :3] = black
    assert (got[:7, :, :, :3] == black).all() and not got[..., 3:].any() and (got[7, :, :, :3] != black).any()
    cols = colour_with(np.broadcast_to(col[0], (B, 8)), np.arange(B) % 6)
    out = run_image(imgs, sz, mats, cols, (24, 40), False)
    want = check_colour("outside / non-finite", out, imgs, sz, mats, cols, (24, 40), False)
    for b in range(6):                                               # every pixel is the colour chain of the black pixel: one value per channel
        assert (out[b, :, :, :3] == out[b, 0, 0, :3]).all() and np.array_equal(out[b], want[b]), b
    assert not np.isnan(cc.colour(np.zeros((2, 2, 3), np.float32), cols[0], MEAN, STD)["y"]).any()


def test_an_order_outside_0_5_skips_the_three_functions():
    img, sizes, mat, col = image_problem()
    bad = colour_with(col, (6.0, -1.0, np.nan))
    got = run_image(img, sizes, mat, bad, (24, 40), False)
    check_colour("order outside 0..5", got, img, sizes, mat, bad, (24, 40), False)
    light = np.array(col)
    light[:, :3], light[:, 6] = 1.0, 0.0                             # the three functions with alpha 1 change nothing but roundings
    ndiff, worst = cc.bf16_differences(got, run_image(img, sizes, mat, light, (24, 40), False))
    assert worst <= 1 and ndiff * 100 <= got.size


def test_equal_across_calls_streams_and_the_scratch_pool():
    from minddet_amd import det_ops

    img, sizes, mat, col = image_problem()
    col = colour_with(col, (4, 0, 3))
    d = [dev(a) for a in (img, sizes, mat, col)]

    def garbage():
        out = torch.empty((3, 40, 56, 4), dtype=torch.bfloat16, device=DEV)
        out.view(torch.uint8).fill_(0xFF)
        return out

    first = bits16(det_ops.cn_aug_image(d[0], d[1], d[2], MEAN, STD, (24, 40), colour=d[3], out=garbage()))
    again = bits16(det_ops.cn_aug_image(d[0], d[1], d[2], MEAN, STD, (24, 40), colour=d[3], out=garbage()))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs, pool = [garbage(), garbage()], [garbage(), garbage()]
    torch.cuda.synchronize()
    for rep in range(2):                                             # the second round reuses each stream's pool buffer
        for s, o, q in zip(streams, outs, pool):
            with torch.cuda.stream(s):
                det_ops.cn_aug_image(d[0], d[1], d[2], MEAN, STD, (24, 40), colour=d[3], out=o)
                det_ops.cn_aug_image(d[0], d[1], d[2], MEAN, STD, (24, 40), colour=d[3], out=q, workspace=False)
    for o in [again] + [bits16(o) for o in outs + pool]:
        assert np.array_equal(first, o)                              # (a surviving 0xFF byte would differ from `first`)
    check_colour("calls and streams", first, img, sizes, mat, col, (24, 40), True)
    f = fixture()
    t1 = det_ops.cn_aug_transform(dev(f["size"][::2]), dev(f["draws"][::2]), **attrs_of(f, 0))
    with torch.cuda.stream(streams[0]):
        t2 = det_ops.cn_aug_transform(dev(f["size"][::2]), dev(f["draws"][::2]), **attrs_of(f, 0))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(t1, t2))


def test_the_flip_folded_into_the_matrix_equals_the_flipped_image():
    """s = 64 x 0.75 = 48 on a 32-wide input: r = 1.5, every source position a multiple of 0.5, so every product and sum of the sampler is
    exact and the two ways give the same bits: the stored image with the flipped draw, and the image flipped on the host with the
    draw whose centre is already the mirrored one"""
    from minddet_amd import det_ops

    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (1, 64, 64, 3), dtype=np.uint8)
    size = np.array([(64, 64)], np.int32)
    kw = dict(rand_crop=True, input_hw=(24, 32), down_ratio=4, **ATTRS)
    a = cc.transform(size, np.array([(0.75, 30.0, 20.0, 0.0)]), **kw)
    b = cc.transform(size, np.array([(0.75, 33.0, 20.0, 0.9)]), **kw)
    assert a["flipped"][0] and not b["flipped"][0] and np.array_equal(a["c"], b["c"]) and a["mat_in"][0].tolist() == [-1.5, 0, 54, 0, 1.5, 2]
    col = np.array([(1.3, 0.7, 1.2, 0.01, -0.02, 0.03, 3, 0)])
    for c in (None, col):
        ma, _, fw = det_ops.cn_aug_transform(dev(size), dev(np.array([(0.75, 30.0, 20.0, 0.0)])), **kw)
        mb, _, _ = det_ops.cn_aug_transform(dev(size), dev(np.array([(0.75, 33.0, 20.0, 0.9)])), **kw)
        one = bits16(det_ops.cn_aug_image(dev(img), dev(size), ma, MEAN, STD, (24, 32), colour=None if c is None else dev(c), stem_layout=False))
        two = bits16(det_ops.cn_aug_image(dev(img[:, :, ::-1]), dev(size), mb, MEAN, STD, (24, 32), colour=None if c is None else dev(c), stem_layout=False))
        assert int(fw[0]) == 64 and np.array_equal(one, two) and len(np.unique(one)) > 100


@functools.lru_cache(maxsize=None)
def tiny_net(**augment):
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centernet", "centernet_tiny_train.py"))
    train_cfg = dict(cfg.train_cfg, augment=dict(cfg.train_cfg["augment"], **augment))
    return build_detector(cfg.model, train_cfg, cfg.test_cfg).to(DEV), train_cfg


def tiny_batch():
    rng = np.random.default_rng(21)
    sizes = np.array([(120, 160), (90, 200)], np.int32)
    img = np.full((2, 120, 200, 3), 255, np.uint8)
    for b, (h, w) in enumerate(sizes):
        img[b, :h, :w] = rng.integers(0, 256, (h, w, 3))
    c = rng.uniform(20, 100, (2, 6, 2)) * (1.4, 0.9)
    s = rng.uniform(10, 60, (2, 6, 2))
    boxes = np.concatenate([c - s / 2, c + s / 2], -1).astype(np.float32)
    classes = rng.integers(1, 6, (2, 6)).astype(np.int32)
    return img, sizes, boxes, classes


def test_train_example_equals_the_targets_of_the_contracts_matrices():
    net, train_cfg = tiny_net()
    img, sizes, boxes, classes = tiny_batch()
    aug = net.augment_op()
    assert aug is net.augment_op() and net.targets_op() is net.targets_op() and not aug.stem_layout and aug.input_hw == (64, 96)
    gen = torch.Generator(device=DEV).manual_seed(5)
    draws, colour = aug.draw(dev(sizes), gen)
    inp, ex = net.train_example(dev(img), dev(sizes), dev(boxes), dev(classes), draws=draws, colour=colour)
    torch.cuda.synchronize()
    a = train_cfg["augment"]
    want = cc.transform(sizes, draws.cpu().numpy(), rand_crop=a["rand_crop"], scale=a["scale"], shift=a["shift"], flip_prop=a["flip_prop"],
                        input_hw=(64, 96), down_ratio=4)
    assert np.array_equal(ex["trans_out"].cpu().numpy(), want["trans_out"]) and np.array_equal(ex["flip_width"].cpu().numpy(), want["flip_width"])
    direct = net.targets_op()(dev(boxes), dev(classes), trans=dev(want["trans_out"]), flip_width=dev(want["flip_width"]))
    for k in ("hm", "ind", "reg_mask", "wh", "reg"):
        assert torch.equal(ex[k], direct[k]), k
    assert inp.shape == (2, 64, 96, 8) and inp.dtype == torch.bfloat16 and ex["hm"].shape == (2, 5, 16, 24)
    check_colour("tiny config", bits16(inp), img, sizes, want["mat_in"], colour.cpu().numpy(), (64, 96), False)
    inp2, ex2 = net.train_example(dev(img), dev(sizes), dev(boxes), dev(classes), generator=torch.Generator(device=DEV).manual_seed(5))
    assert torch.equal(inp2.view(torch.int16), inp.view(torch.int16)) and torch.equal(ex2["hm"], ex["hm"])      # the same seed: the same draws


def test_train_loss_is_finite_and_repeats_bit_for_bit():
    net, _ = tiny_net()
    img, sizes, boxes, classes = tiny_batch()
    draws, colour = net.augment_op().draw(dev(sizes), torch.Generator(device=DEV).manual_seed(6))
    runs = [net.train_loss(dev(img), dev(sizes), dev(boxes), dev(classes), draws=draws, colour=colour, grad=True) for _ in range(2)]
    torch.cuda.synchronize()
    one, two = runs
    assert set(one) == {"total", "parts", "num_pos", "grad", "head", "example"} and one["grad"].shape == (2, 16, 24, 16)
    for k in ("total", "parts", "num_pos", "grad"):
        assert bool(torch.isfinite(one[k]).all()) and torch.equal(one[k], two[k]), k
    assert torch.equal(one["head"].view(torch.int16), two["head"].view(torch.int16)) and float(one["total"]) > 0 and bool(one["grad"].any())
    fwd = net.train_loss(dev(img), dev(sizes), dev(boxes), dev(classes), draws=draws, colour=colour)
    assert "grad" not in fwd and torch.equal(fwd["total"], one["total"])


def test_train_loss_without_augmentation_equals_loss_on_image_preprocess():
    from minddet_amd import det_ops, nn_ops

    net, _ = tiny_net(flip_prop=0.0, color_aug=False, rand_crop=False)
    _, _, boxes, classes = tiny_batch()
    img = np.random.default_rng(3).integers(0, 256, (2, 120, 200, 3), dtype=np.uint8)
    sizes = np.array([(120, 200)] * 2, np.int32)
    draws = torch.zeros((2, 4), dtype=torch.float64, device=DEV)
    got = net.train_loss(dev(img), dev(sizes), dev(boxes), dev(classes), draws=draws, grad=True)
    mat_in, trans_out, flip_width = det_ops.cn_aug_transform(dev(sizes), draws, rand_crop=False, scale=0.4, shift=0.1, flip_prop=0.0, input_hw=(64, 96),
                                                             down_ratio=4)
    x = nn_ops.image_preprocess(dev(img), mat_in, MEAN, STD, (64, 96), stem_layout=False)
    example = net.targets_op()(dev(boxes), dev(classes), trans=trans_out, flip_width=flip_width)
    want = net.loss(x, example, grad=True)
    torch.cuda.synchronize()
    assert not bool(flip_width.any()) and float(want["num_pos"]) >= 4
    for k in ("total", "parts", "num_pos", "grad"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["head"].view(torch.int16), want["head"].view(torch.int16))


def test_draws_on_the_device():
    from minddet_amd import det_ops

    rng = np.random.default_rng(12)
    B = 1200
    sizes = np.stack([rng.integers(1, 701, B), rng.integers(1, 901, B)], 1).astype(np.int32)
    sizes[:4] = [(1, 1), (2, 2), (255, 256), (257, 300)]
    s = dev(sizes)
    gen = torch.Generator(device=DEV).manual_seed(77)
    aug = det_ops.CenterNetAugment((64, 96), 4)
    draws, colour = aug.draw(s, gen)
    assert draws.is_cuda and colour.is_cuda and draws.dtype == colour.dtype == torch.float64
    d, c = draws.cpu().numpy(), colour.cpu().numpy()
    assert set(d[:, 0].tolist()) == set(np.arange(0.6, 1.4, 0.1).tolist())
    for col, k in ((1, 1), (2, 0)):                                  # randint(border, size - border) per sample size
        size = sizes[:, k].astype(np.int64)
        lo = det_ops.CenterNetAugment.get_border(128, torch.from_numpy(size)).numpy()
        assert (d[:, col] == np.round(d[:, col])).all() and (d[:, col] >= lo).all() and (d[:, col] < np.maximum(size - lo, lo + 1)).all()
        wide = size >= 600
        assert d[wide, col].min() < 200 and d[wide, col].max() > size[wide].max() - 200      # the interval is used, both ends
    assert d[0, 1] == 0 and d[0, 2] == 0 and (d[:, 3] >= 0).all() and (d[:, 3] < 1).all() and 0.4 < (d[:, 3] < 0.5).mean() < 0.6
    assert (c[:, :3] >= 0.6).all() and (c[:, :3] <= 1.4).all() and c[:, :3].std() > 0.2 and not c[:, 7].any()
    assert set(c[:, 6].tolist()) == {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}
    # lighting: eig_vec . (eig_val * N(0, 0.1)): its covariance is eig_vec diag((0.1 eig_val)^2) eig_vec^T
    cov = aug.eig_vec @ np.diag((0.1 * aug.eig_val) ** 2) @ aug.eig_vec.T
    assert np.allclose(np.cov(c[:, 3:6].T), cov, rtol=0.25, atol=0.1 * cov.max())
    plain, none = det_ops.CenterNetAugment((64, 96), 4, rand_crop=False, color_aug=False).draw(s, gen)
    n = plain[:, :3].cpu().numpy()
    assert none is None and n.size == 3600 and abs(n.std(ddof=1) - 1.0) < 0.1 and abs(n.mean()) < 0.1
    again, _ = aug.draw(s, torch.Generator(device=DEV).manual_seed(77))
    assert torch.equal(again, draws)
