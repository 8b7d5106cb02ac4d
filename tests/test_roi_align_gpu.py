"""-m gpu: md_roi_align on both of its kernels -- roi_align_c32_kernel (C % 32 == 0: every detector's C = 256; with sampling 2 the
separable form that merges duplicate rows / columns) and roi_align_kernel (other C) -- against the float64-accumulating reference
np_ops.roi_align_fast(acc_dtype=np.float64), EVERY output of every RoI compared.  The kernel a case runs is fixed by its C.

Tolerance, per output:  |got - ref| <= 2^-8 |ref| + 2^-10 M,  M = the largest |feature| among the taps of the bin's in-range samples.
  * 2^-8 |ref|: the output is rounded once to bf16 (8 significant bits, round to nearest: at most half an ulp = 2^-8 relative).
  * 2^-10 M: everything else, each term far smaller: the fp32 bilinear weights and their products (a few 2^-24 relative), the fp32
    summation order of the up to 16 taps (the separable form sums merged weights), and sample coordinates that differ by a few fp32
    ulps where hipcc contracts y1 + ph * bh into an FMA (coordinates reach 336 px on P2, where one ulp is 2^-15 px, so a weight moves
    by about 2^-13 and the tap it weights by at most 2 M).
  One wrong tap is far outside this bound: a bilinear weight off by w moves the output by w |feature| / g^2, and a sample that
  loses a quarter of its weight already moves it by M / 16 for g = 2.
Sample coordinates sit exactly on the -1 / H / W discontinuities (in range or not) only in the edge-geometry cases, whose corners
are dyadic and whose bin widths are multiples of 3 * 2^-k at the level, so every coordinate is exact in fp32 (FMA or not) and kernel
and reference take the same decision; random RoIs are kept 1e-3 px away from them.  The FPN level indices are bit-exact against
np_ops.fpn_level."""
import numpy as np
import pytest
import torch

from oracle import np_ops
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
STRIDES = (4, 8, 16, 32)


def kernel_for(C):
    """md_roi_align's dispatch: C % 32 == 0 -> roi_align_c32_kernel, else roi_align_kernel (C % 8 == 0)"""
    return "c32" if C % 32 == 0 else "generic"


def bf16_feats(rng, N, shapes, C):
    """[N,H,W,C] bf16 levels (device) and their exact fp32 values (host)"""
    dev, host = [], []
    for (h, w) in shapes:
        t = torch.from_numpy(rng.normal(0, 1, (N, h, w, C)).astype(np.float32)).to(torch.bfloat16)
        dev.append(t.to(DEV))
        host.append(t.float().numpy())
    return dev, host


def samples_1d(lo, hi, scale, P, g, aligned):
    """the kernels' fp32 sample coordinates along one axis: [R, P * g]"""
    off = np.float32(0.5 if aligned else 0.0)
    a, b = lo.astype(np.float32) * np.float32(scale) - off, hi.astype(np.float32) * np.float32(scale) - off
    r = b - a
    if not aligned:
        r = np.maximum(r, np.float32(1))
    bsz = r / np.float32(P)
    p = np.repeat(np.arange(P, dtype=np.float32), g)
    i = np.tile(np.arange(g, dtype=np.float32), P)
    return a[:, None] + p[None, :] * bsz[:, None] + (i[None, :] + np.float32(0.5)) * bsz[:, None] / np.float32(g)


def away_from_edges(rois, shapes, P, g, aligned, eps=1e-3):
    """RoIs none of whose sample coordinates lies within eps px of -1, H or W at the RoI's level"""
    lv = np_ops.fpn_level(rois[:, 1:], k_max=1 + len(shapes)) - 2
    ok = np.ones(len(rois), bool)
    for l, (h, w) in enumerate(shapes):
        m = lv == l
        s = 1.0 / STRIDES[l]
        for c, size in ((samples_1d(rois[m, 1], rois[m, 3], s, P, g, aligned), w), (samples_1d(rois[m, 2], rois[m, 4], s, P, g, aligned), h)):
            ok[np.flatnonzero(m)] &= (np.minimum(np.abs(c + 1), np.abs(c - size)) > eps).all(1)
    return rois[ok]


def check(feats_dev, feats_host, rois, P, g, aligned, scales=None):
    """run md_roi_align and compare every output of every RoI with the float64 reference at the RoI's level"""
    from minddet_amd import det_ops

    L = len(feats_dev)
    scales = [1.0 / s for s in STRIDES[:L]] if scales is None else scales
    out, lv = det_ops.roi_align(feats_dev, torch.from_numpy(rois).to(DEV), P, scales, g, aligned, return_levels=True)
    out, lv = out.float().cpu().numpy(), lv.cpu().numpy()
    np.testing.assert_array_equal(lv, np_ops.fpn_level(rois[:, 1:], k_max=1 + L))
    worst = 0.0
    for l in range(L):
        for b in range(feats_host[l].shape[0]):
            idx = np.flatnonzero((lv == l + 2) & (rois[:, 0].astype(np.int64) == b))
            if idx.size == 0:
                continue
            ref, M = np_ops.roi_align_fast(feats_host[l][b].transpose(2, 0, 1), rois[idx, 1:], P, scales[l], g, aligned,
                                           acc_dtype=np.float64, return_tap_max=True)
            ref, M = ref.transpose(0, 2, 3, 1), M.transpose(0, 2, 3, 1).astype(np.float64)
            err = np.abs(out[idx].astype(np.float64) - ref)
            tol = 2.0 ** -8 * np.abs(ref) + 2.0 ** -10 * M
            bad = err > tol
            if bad.any():
                r, ph, pw, c = np.argwhere(bad)[0]
                raise AssertionError(f"{bad.sum()} outputs out of tolerance (level {l}, image {b}); first: RoI {idx[r]} {rois[idx[r]]} bin "
                                     f"({ph},{pw}) channel {c}: got {out[idx[r], ph, pw, c]} ref {ref[r, ph, pw, c]} M {M[r, ph, pw, c]}")
            worst = max(worst, float((err / np.maximum(tol, 1e-30)).max()))
    return lv, worst


def random_rois(rng, R, N, img_hw=(800, 1344), lo=8.0, hi=1000.0, clip=True):
    """RoIs whose sqrt(area) is log-uniform in [lo, hi] (so every FPN level gets some), aspect 1:2 .. 2:1, batch index uniform"""
    s = np.exp(rng.uniform(np.log(lo), np.log(hi), R))
    ar = np.exp(rng.uniform(np.log(0.5), np.log(2.0), R))
    w, h = s * np.sqrt(ar), s / np.sqrt(ar)
    cx, cy = rng.uniform(0, img_hw[1], R), rng.uniform(0, img_hw[0], R)
    x1, y1, x2, y2 = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
    if clip:   # proposals are clipped to the image (delta2bbox max_shape)
        x1, x2 = np.clip(x1, 0, img_hw[1] - 1), np.clip(x2, 1, img_hw[1])
        y1, y2 = np.clip(y1, 0, img_hw[0] - 1), np.clip(y2, 1, img_hw[0])
    return np.stack([rng.integers(0, N, R), x1, y1, x2, y2], 1).astype(np.float32)


PYRAMID = [(200, 336), (100, 168), (50, 84), (25, 42)]   # an 800 x 1344 input at strides 4..32


def test_production_box_head_and_mask_head():
    """Faster / Mask R-CNN: batch 2, 800 x 1344, C 256, sampling 2, aligned; P 7 over 1000 RoIs per image spread over P2-P5 (the box
    head), then P 14 over 100 RoIs per image (the mask head)"""
    assert kernel_for(256) == "c32"
    rng = np.random.default_rng(0)
    fd, fh = bf16_feats(rng, 2, PYRAMID, 256)
    rois = away_from_edges(random_rois(rng, 2000, 2), PYRAMID, 7, 2, True)
    assert len(rois) > 1950
    lv, worst = check(fd, fh, rois, 7, 2, True)
    assert all((lv == k).sum() > 100 for k in (2, 3, 4, 5)), np.bincount(lv)
    rois = away_from_edges(random_rois(rng, 200, 2), PYRAMID, 14, 2, True)
    check(fd, fh, rois, 14, 2, True)
    print(f"production RoIAlign: worst |err| / tolerance {worst:.3f}")


SMALL = [(50, 84), (25, 42), (13, 21), (7, 11)]   # a 200 x 336 input


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("g", [2, 1, 3])
@pytest.mark.parametrize("C,kernel", [(32, "c32"), (96, "c32"), (256, "c32"), (8, "generic"), (24, "generic"), (40, "generic")])
def test_both_kernels_every_sampling_and_alignment(C, kernel, g, aligned):
    """C 32 / 96 (an odd number of 32-channel groups) / 256 run the C32 kernel, C 8 / 24 / 40 the generic one; sampling 2 (the
    separable, deduplicating form on the C32 kernel), 1 and 3; aligned and not.  RoIs from sub-pixel to larger than the map, partly
    outside it (not clipped), over two images."""
    assert kernel_for(C) == kernel
    rng = np.random.default_rng(C * 10 + g + 100 * aligned)
    fd, fh = bf16_feats(rng, 2, SMALL, C)
    R = 60 if C >= 96 else 150
    rois = random_rois(rng, R, 2, img_hw=(200, 336), lo=1.0, hi=600.0, clip=False)
    rois = away_from_edges(rois, SMALL, 7, g, aligned)
    assert len(rois) > 0.9 * R
    check(fd, fh, rois, 7, g, aligned)


def edge_rois(g, H, W):
    """RoIs in LEVEL coordinates (x1, y1, x2, y2) whose every sample coordinate is exact in fp32 for sampling g <= 3 (dyadic corners,
    bin widths multiples of 3 * 2^-k): each lands where it is meant to, the same in kernel and reference."""
    sub = 0.1875                 # bin width 3/16 px: 7 bins span 1.3125 px, so the 2 x 2 samples of neighbouring bins share rows / columns
    half = 0.5 * sub / g         # offset of a bin's first sample
    c = []
    c.append((3.0, 2.0, 3.0 + 7 * sub, 2.0 + 7 * sub))                        # sub-pixel bins (the deduplication merge)
    c.append((5.5, 4.25, 5.5 + 7 * 0.375, 4.25 + 7 * 0.75))                   # bins of 3/8 and 3/4 px
    c.append((0.5, 1.5, 0.5 + 7.0 * g, 1.5 + 7.0 * g))                       # bins of g px: every sample on integer coordinates (weight 0)
    c.append((-1.0, -1.0, -1.0 + 7 * sub, -1.0 + 7 * sub))                    # samples in [-1, 0)
    c.append((-1.0 - half, -1.0 - half, -1.0 - half + 7 * sub, -1.0 - half + 7 * sub))   # first sample exactly at -1 (in range)
    c.append((-1.0 - 2 * half, 2.0, -1.0 - 2 * half + 7 * sub, 2.0 + 7 * sub))            # first sample just below -1 (out)
    c.append((W - half, H - half, W - half + 7 * sub, H - half + 7 * sub))    # first sample exactly at (W, H): in range, clamped
    last = (7 - 1 + (g - 0.5) / g) * sub
    c.append((W - last, H - last, W - last + 7 * sub, H - last + 7 * sub))    # last sample exactly at (W, H)
    c.append((W - 1.5, H - 1.5, W - 1.5 + 7 * sub, H - 1.5 + 7 * sub))        # across the H-1 / W-1 clamps
    c.append((W - 2.0, H - 2.0, W - 2.0 + 7 * 0.75, H - 2.0 + 7 * 0.75))      # from inside to past W / H
    c.append((-4.0, 8.0, -4.0 + 10.5, 8.0 + 10.5))                            # partly outside
    c.append((W + 2.0, -15.0, W + 2.0 + 5.25, -15.0 + 5.25))                  # wholly outside
    c.append((-9.0, -9.0, -9.0 + 5.25, -9.0 + 5.25))                          # wholly outside, up-left
    c.append((5.25, 3.5, 5.25, 3.5))                                          # zero size
    c.append((9.0, 6.0, 9.0 - 10.5, 6.0 - 5.25))                              # inverted
    c.append((-2.5, -3.0, -2.5 + 7 * 3.75, -3.0 + 7 * 3.0))                   # larger than the map
    return np.asarray(c, np.float64)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("g", [2, 1, 3])
@pytest.mark.parametrize("C,kernel", [(32, "c32"), (24, "generic")])
def test_edge_geometry(C, kernel, g, aligned):
    """Both kernels (C 32 and 24), one level (stride 4) of a batch of N = 3: sub-pixel bins, samples on integer coordinates, in
    [-1, 0), exactly at -1 / H / W and just past them, across the H-1 / W-1 clamps, RoIs partly or wholly outside the map, zero-size
    and inverted; every case on image 1 (a wrong image stride shows) and on images 0 and 2"""
    assert kernel_for(C) == kernel
    rng = np.random.default_rng(C + g + 10 * aligned)
    H, W = 12, 20
    fd, fh = bf16_feats(rng, 3, [(H, W)], C)
    lvl = edge_rois(g, H, W)
    off = 0.5 if aligned else 0.0
    img = (lvl + off) * 4.0                       # exact: level coordinate = img / 4 - off
    rois = np.concatenate([np.concatenate([np.full((len(img), 1), b), img], 1) for b in (1, 0, 2)], 0).astype(np.float32)
    assert (((rois[:, 1:].astype(np.float64) / 4.0 - off) == np.tile(lvl, (3, 1)))).all()
    check(fd, fh, rois, 7, g, aligned, scales=[0.25])
    # the cases really reach the edges: samples exactly at -1 and at W (x), and every output of the wholly-outside RoIs is 0
    xs = samples_1d(rois[:len(lvl), 1], rois[:len(lvl), 3], 0.25, 7, g, aligned)
    assert (xs == -1.0).any() and (xs == W).any() and ((xs > -1.0) & (xs < 0.0)).any()
