"""-m gpu: md_paste_masks (csrc/twostage.hip) against the float64 judge of the public definition (tests/paste_contract.py), alone: no
fp32 twin stands between the device and the definition here (the bit-for-bit twin comparison stays in tests/test_mask_rcnn_gpu.py; it is
repeated below only for the constant-threshold masks, which the band leaves wholly free).

Every call goes through the C ABI into an output that lies inside a sentinel-filled buffer with guard zones on both sides, twice, with
two different sentinels (0xA5 and 0x5A bytes): the guards must stay intact and the two outputs must be byte-equal, so no element can
have been left unwritten.  Both output forms are judged, the bit form on its raw words (padding bits of a ragged last word included).
A decision must equal the judge's wherever the float64 value lies outside the derived band; in the exact-regime cases on every pixel.

Measured on the MI355X (band and CAP as fixed in tests/paste_contract.py beforehand; every test prints these figures again):
  free share (decisions inside the band / decisions inside the support), in-band pixels where device != judge
    95 'free' cases: free share 0 in 92; uniform-6x100-S32-t0.5 2.0e-4 (1 of 4 965), uniform-75x101-S14-t0.25 1.8e-5,
                     uniform-75x101-S56-t0.503906 2.1e-5; in-band disagreements 0 in every case
    18 exact-regime cases: free share 0 by construction, equal on every pixel, planted equalities included
    const_hi / const_lo (thr +- 2^-20): free share 0, every interior pixel on / off
    const_eq (mask == thr): free share 0.92 / 0.68 / 0.95, in-band disagreements 0, device == fp32 twin bit for bit
    production 800 x 1344, R = 16: free share 1.7e-6 (2 of 1 190 517), in-band disagreements 0; R = 128: every row equal to its pair's
    tiny Mask R-CNN, forward(paste=True): free share 3.1e-5 (2 of 64 698), in-band disagreements 0
  no decision outside the band differed; all guards intact.
"""
import numpy as np
import pytest
import torch

from tests import paste_contract as pc
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
GUARD = 4096                       # bytes on each side of the output
SENTINELS = (0xA5, 0x5A)

def _launch(masks, dets, H, W, thr, bits, fill, stream=None):
    """one md_paste_masks call into a guarded, sentinel-filled output -> the output's bytes (numpy)"""
    from minddet_amd import _lib, det_ops

    R, Ww = masks.shape[0], (W + 31) // 32
    nbytes = R * H * (Ww * 4 if bits else W)
    flat = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=DEV)
    body = flat[GUARD:GUARD + nbytes]
    out = body.view(torch.int32).view(R, H, Ww) if bits else body.view(R, H, W)
    torch.cuda.synchronize()
    _lib.call("md_paste_masks", [masks, dets, out], extra=det_ops._PasteAttrs(H, W, float(thr), int(bits)),
              stream=None if stream is None else stream.cuda_stream)
    torch.cuda.synchronize()
    assert bool((flat[:GUARD] == fill).all()) and bool((flat[GUARD + nbytes:] == fill).all()), "write outside the output tensor"
    return body.cpu().numpy()


def _paste(masks, dets, H, W, thr):
    """both forms, each run with both sentinels -> (words [R,H,Ww] uint32, u8 [R,H,W] uint8)"""
    md, dd = torch.from_numpy(masks).to(DEV), torch.from_numpy(dets).to(DEV)
    R, Ww = masks.shape[0], (W + 31) // 32
    got = []
    for bits in (True, False):
        a, b = (_launch(md, dd, H, W, thr, bits, fill) for fill in SENTINELS)
        assert np.array_equal(a, b), "an output element kept its sentinel" + (" (or the bit form is not deterministic)" if bits else "")
        got.append(a)
    words, u8 = got[0].view(np.uint32).reshape(R, H, Ww), got[1].reshape(R, H, W)
    assert u8.max(initial=0) <= 1, "uint8 form: a byte that is neither 0 nor 1"
    bitsv = pc.unpack_bits(words)
    assert not bitsv[..., W:].any(), "bit form: a bit at a position >= W is set"
    assert np.array_equal(bitsv[..., :W], u8), "the bit form and the uint8 form disagree"
    return words, u8


def _judge(name, words, u8, judged, W, exact=False, cap=True):
    """device against judge: equal outside the band (everywhere if exact), raw words included; -> (free share, in-band disagreements)"""
    v, s, dec, free = judged
    bad = (u8 != dec) & ~free
    assert not bad.any(), f"{name}: {int(bad.sum())} decisions differ from the judge outside the band; first at {np.argwhere(bad)[0]}, " \
                          f"value {v[bad][0]!r}"
    open_words = pc.pack_bits(free.astype(np.uint8), W)
    assert np.array_equal(words & ~open_words, pc.pack_bits(dec, W) & ~open_words), f"{name}: raw words differ from the judge's"
    share, inband = float(free.sum()) / max(int(s.sum()), 1), int(((u8 != dec) & free).sum())
    print(f"{name}: support {int(s.sum())}, free share {share:.2e}, in-band device != judge {inband}")
    if exact:
        assert not free.any()
    if cap:
        assert share <= pc.CAP, (name, share)
    return share, inband


@pytest.mark.parametrize("kind", ["free", "exact", "const"])
def test_small_cases_against_the_judge(kind):
    n = 0
    for c in pc.small_cases():
        if not c.kind.startswith(kind):
            continue
        words, u8 = _paste(c.masks, c.dets, c.H, c.W, c.thr)
        _judge(c.name, words, u8, c.judged, c.W, exact=c.kind == "exact", cap=c.kind in ("free", "exact"))
        for r in c.must_be_empty:
            assert not words[r].any(), (c.name, r)
        if c.kind.startswith("const"):
            from oracle import np_ops

            inner, free = c.interior(), c.judged[3]
            if c.kind == "const_hi":
                assert u8[inner & ~free].all(), c.name
            elif c.kind == "const_lo":
                assert not u8[inner].any(), c.name
            np.testing.assert_array_equal(u8, np_ops.paste_masks(c.masks, c.dets, (c.H, c.W), c.thr), err_msg=c.name)
        n += 1
    assert n >= 9


def test_thresholds_paste_the_support_or_nothing():
    seen = set()
    for c in pc.small_cases():
        if c.kind != "free" or c.thr in pc.THRESHOLDS[:3]:
            continue
        _, s, _, free = c.judged
        _, u8 = _paste(c.masks, c.dets, c.H, c.W, c.thr)
        if c.thr <= 0:                       # the support and nothing outside it
            assert s.any() and np.array_equal(u8[~free], s[~free].astype(np.uint8)), c.name
        else:                                # 1.0 against masks below 1, 1.5, NaN: nothing
            assert not u8.any(), c.name
        seen.add(repr(c.thr))
    assert len(seen) == 5


def test_memory_the_kernel_must_not_read():
    """NaN in the mask rows of empty slots and in the label column changes nothing"""
    c = next(c for c in pc.small_cases() if c.name.startswith("uniform-75x101-S28"))
    words, u8 = _paste(c.masks, c.dets, c.H, c.W, c.thr)
    masks, dets = c.masks.copy(), c.dets.copy()
    dead = [r for r in range(len(dets)) if not pc._row_valid(dets[r].astype(np.float64))]
    assert len(dead) >= 8 and len(dead) < len(dets)
    masks[dead] = np.nan
    dets[:, 5] = np.nan
    words2, u82 = _paste(masks, dets, c.H, c.W, c.thr)
    assert np.array_equal(words, words2) and np.array_equal(u8, u82)
    assert not words2[dead].any() and words2.any()


def _production_rows(rng, n, H, W, S):
    bw, bh = np.exp(rng.uniform(np.log(2.0), np.log(1.2 * W), n)), np.exp(rng.uniform(np.log(2.0), np.log(1.2 * H), n))
    cx, cy = rng.uniform(0, W, n), rng.uniform(0, H, n)
    boxes = np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1)
    boxes[0] = (-0.5, -0.25, W + 0.5, H + 0.25)
    masks = np.concatenate([pc._blob_masks(rng, n - n // 2, S), pc._uniform_masks(rng, n // 2, S)])
    return masks.astype(np.float32), pc._dets(boxes, rng)


def test_production_shape_bit_form():
    """800 x 1344, bit form (what graphs.MaskRCNN runs): 16 rows, every one judged; then 128 rows that are a shuffle of 8 distinct
    (mask, box) pairs -- 128 * 800 * 42 work items pass the kernel's 16 384 x 256 grid-stride limit -- every row compared; two calls and
    a call on a second stream are bit-identical."""
    H, W, S, thr = 800, 1344, 28, 0.5
    rng = np.random.default_rng(77)
    masks, dets = _production_rows(rng, 16, H, W, S)
    c = pc.Case("production-800x1344-R16", H, W, masks, dets, thr)
    md, dd = torch.from_numpy(masks).to(DEV), torch.from_numpy(dets).to(DEV)
    a, b = (_launch(md, dd, H, W, thr, True, fill) for fill in SENTINELS)
    on_second = _launch(md, dd, H, W, thr, True, SENTINELS[0], stream=torch.cuda.Stream(device=DEV))
    assert np.array_equal(a, b) and np.array_equal(a, on_second)
    words = a.view(np.uint32).reshape(16, H, W // 32)
    _judge(c.name, words, pc.unpack_bits(words), c.judged, W)

    R = 128
    assert R * H * (W // 32) > 16384 * 256
    pick = rng.permutation(np.arange(R) % 8)
    m8, d8 = masks[:8][pick], dets[:8][pick]
    md, dd = torch.from_numpy(m8).to(DEV), torch.from_numpy(d8).to(DEV)
    a, b = (_launch(md, dd, H, W, thr, True, fill) for fill in SENTINELS)
    assert np.array_equal(a, b)
    big = a.view(np.uint32).reshape(R, H, W // 32)
    for r in range(R):
        assert np.array_equal(big[r], words[pick[r]]), f"row {r} (pair {pick[r]})"


def test_determinism_small_both_forms():
    c = next(c for c in pc.small_cases() if c.name.startswith("blob-5x101"))
    md, dd = torch.from_numpy(c.masks).to(DEV), torch.from_numpy(c.dets).to(DEV)
    side = torch.cuda.Stream(device=DEV)
    for bits in (True, False):
        a = _launch(md, dd, c.H, c.W, c.thr, bits, SENTINELS[0])
        assert np.array_equal(a, _launch(md, dd, c.H, c.W, c.thr, bits, SENTINELS[0]))
        assert np.array_equal(a, _launch(md, dd, c.H, c.W, c.thr, bits, SENTINELS[1], stream=side))


def test_end_to_end_tiny_mask_rcnn():
    """configs/mask_rcnn/mask_rcnn_tiny.py, forward(paste=True): every detection's pasted words judged from the device's own masks and
    dets; empty slots are zero"""
    from minddet.models import Config, build_detector

    cfg = Config.fromfile("configs/mask_rcnn/mask_rcnn_tiny.py")
    m = build_detector(cfg.model, cfg.train_cfg, cfg.test_cfg).to(DEV)
    g = torch.Generator().manual_seed(0)
    B, H, W = 2, 128, 192
    x = torch.zeros((B, H, W, 8))
    x[..., :3] = torch.randn((B, H, W, 3), generator=g)
    dets, count, masks, pasted = m.forward(x.to(torch.bfloat16).to(DEV), paste=True)
    torch.cuda.synchronize()
    D, S = dets.shape[1], masks.shape[2]
    assert pasted.shape == (B, D, H, W // 32) and pasted.dtype == torch.int32 and int(count.sum()) > 0
    words = pasted.cpu().numpy().view(np.uint32).reshape(B * D, H, W // 32)
    c = pc.Case("tiny-mask-rcnn", H, W, masks.cpu().numpy().reshape(B * D, S, S), dets.cpu().numpy().reshape(B * D, 6), m.mask_thr)
    _judge(c.name, words, pc.unpack_bits(words), c.judged, W)
    cnt = count.cpu().numpy()
    assert words.any()
    for b in range(B):
        assert not words.reshape(B, D, H, -1)[b, cnt[b]:].any()
