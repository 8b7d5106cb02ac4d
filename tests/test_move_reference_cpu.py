"""CPU checks of tests/move_contract.py, the exact references and data generators that tests/test_move_production_gpu.py holds the
pooling, layout and two-stage glue kernels to:

* every reference against an independent public definition on small ragged shapes: the max references against F.max_pool2d (explicit
  F.pad for zero_pad), the SPPF reference against three chained F.max_pool2d, md_upsample_add against F.interpolate(mode="nearest",
  size=) + `+` for every (H, W, Ht, Wt) the FPNs of configs/ produce, copies and casts against torch slicing / permute, the glue ops
  against a plain Python loop per element, bf16_rne_bits against torch's own fp32 -> bf16 conversion;
* each generator plants what its docstring claims, so one that silently stops covering a case fails here.

Finding, kept as a test: F.interpolate computes its source index with a float scale and does NOT equal floor(i * n_in / n_out) for
every non-divisible size pair (first pairs: 44 <- 26, 46 <- 14, 82 <- 2).  It does for every production pair (exact halvings).  The
header names the integer formula as md_upsample_add's contract."""
import glob
import os

import pytest
import torch
import torch.nn.functional as F

from tests import move_contract as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cpu"


def _finite_bf16(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (3.0 * torch.randn(shape, generator=g)).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------------------------
# references against public definitions
# ---------------------------------------------------------------------------------------------------------------------------------
def _torch_pool(x, k, s, p, zero_pad):
    xc = x.double().permute(0, 3, 1, 2)
    if zero_pad:
        y = F.max_pool2d(F.pad(xc, (p, p, p, p), value=0.0), k, s, 0)
    else:
        y = F.max_pool2d(F.pad(xc, (p, p, p, p), value=float("-inf")), k, s, 0)
    return y.permute(0, 2, 3, 1)


POOLS = [((2, 37, 53, 16), 3, 2, 1), ((1, 9, 7, 8), 5, 1, 2), ((3, 3, 4, 8), 5, 1, 2), ((2, 25, 42, 8), 1, 2, 0), ((1, 11, 13, 24), 3, 1, 1),
         ((2, 8, 8, 8), 2, 2, 0), ((1, 1, 1, 8), 3, 1, 1), ((1, 20, 21, 8), 7, 3, 3), ((0, 5, 5, 8), 3, 2, 1)]


@pytest.mark.parametrize("shape,k,s,p", POOLS)
@pytest.mark.parametrize("zero_pad", [0, 1])
def test_maxpool_reference(shape, k, s, p, zero_pad):
    (x,), _ = mc.gen_pool(shape, dict(k=k, stride=s, pad=p, zero_pad=zero_pad), 3, DEV)
    got, want = mc.maxpool(x, k, s, p, zero_pad), _torch_pool(x, k, s, p, zero_pad)
    assert got.shape == want.shape and torch.equal(got, want)
    # Gaussian data too: no planted structure at all
    xr = _finite_bf16(shape, 5)
    assert torch.equal(mc.maxpool(xr, k, s, p, zero_pad), _torch_pool(xr, k, s, p, zero_pad))


def test_maxpool_zero_pad_matters():
    """the two modes differ exactly on the all-negative border windows the generator plants"""
    a = dict(k=3, stride=2, pad=1, zero_pad=1)
    (x,), pl = mc.gen_pool((2, 9, 11, 8), a, 1, DEV)
    y1, y0 = mc.maxpool(x, 3, 2, 1, 1), mc.maxpool(x, 3, 2, 1, 0)
    assert bool((y1[..., 0] != y0[..., 0]).any()) and bool((y1 >= y0).all())
    assert bool((y1[:, 0, :, 0] == 0).all()) and bool((y0[:, 0, :, 0] < 0).all())


@pytest.mark.parametrize("shape,k", [((2, 20, 20, 16), 5), ((1, 7, 9, 8), 5), ((2, 13, 6, 8), 3), ((1, 3, 3, 8), 5), ((1, 40, 41, 8), 5)])
def test_sppf_reference(shape, k):
    (x,), _ = mc.gen_pool(shape, dict(k=k, stride=1, pad=k // 2, zero_pad=0), 7, DEV, sppf_radius=k // 2)
    xc = x.double().permute(0, 3, 1, 2)
    want = []
    for _ in range(3):
        xc = F.max_pool2d(xc, k, 1, k // 2)
        want.append(xc.permute(0, 2, 3, 1))
    for g, w in zip(mc.sppf(x, k), want):
        assert torch.equal(g, w)
    # the one-launch kernel's view: the chain is the max over the (2R+1)^2, (4R+1)^2 and (6R+1)^2 windows
    R = k // 2
    for j, g in enumerate(mc.sppf(x, k)):
        kk = 2 * R * (j + 1) + 1
        assert torch.equal(g, _torch_pool(x, kk, 1, kk // 2, 0))


def production_fpn_pairs():
    """(H, W, Ht, Wt) of every top-down step of every FPN model of configs/, from the config's input size"""
    from minddet.models import Config
    pairs = set()
    for path in sorted(glob.glob(os.path.join(ROOT, "configs", "*", "*.py"))):
        cfg = Config.fromfile(path)
        if cfg.model.get("neck", {}).get("type") != "FPN":
            continue
        h, w = cfg.data["input_hw"]
        lv = []
        for _ in range(5):                  # strides 2 .. 32: every stride-2 stage of the ResNet maps n -> ceil(n / 2)
            h, w = (h + 1) // 2, (w + 1) // 2
            lv.append((h, w))
        for (hh, ww), (ht, wt) in zip(lv[1:-1], lv[2:]):
            pairs.add((hh, ww, ht, wt))
    return sorted(pairs)


def _interp_add(lat, top):
    up = F.interpolate(top.double().permute(0, 3, 1, 2), size=lat.shape[1:3], mode="nearest").permute(0, 2, 3, 1)
    return (lat.double() + up).to(torch.bfloat16)       # a float64 sum of two bf16 rounds to bf16 like the fp32 sum: move_contract


NONDIV_AGREE = [(37, 53, 19, 27), (9, 11, 4, 5), (7, 7, 7, 7), (10, 10, 3, 1), (33, 65, 16, 32), (25, 42, 13, 21), (5, 3, 2, 2)]
NONDIV_DISAGREE = [(44, 46, 26, 14), (82, 8, 2, 4)]     # F.interpolate's float scale lands one source row / column off


def test_upsample_add_reference():
    prod = production_fpn_pairs()
    assert len(prod) >= 6, prod                        # two input sizes x three top-down steps
    print("production FPN (H, W, Ht, Wt):", prod)
    for (H, W, Ht, Wt) in prod + NONDIV_AGREE:
        c = 8 if H * W > 4000 else 16
        (lat, top), _ = mc.gen_upsample_add([[2, H, W, c], [2, Ht, Wt, c]], 11, DEV)
        got, _ = mc.upsample_add(lat, top)
        assert torch.equal(got, mc.bits16(_interp_add(lat, top))), (H, W, Ht, Wt)


def test_upsample_add_integer_formula_is_the_contract():
    """where F.interpolate and the integer formula part, the reference follows the integer formula (a Python loop per pixel)"""
    for (H, W, Ht, Wt) in NONDIV_DISAGREE:
        (lat, top), _ = mc.gen_upsample_add([[1, H, W, 8], [1, Ht, Wt, 8]], 13, DEV)
        got, _ = mc.upsample_add(lat, top)
        assert not torch.equal(got, mc.bits16(_interp_add(lat, top))), "F.interpolate agrees here after all: move the pair"
        want = torch.empty_like(lat)
        for h in range(H):
            for w in range(W):
                want[0, h, w] = (lat[0, h, w].float() + top[0, (h * Ht) // H, (w * Wt) // W].float()).to(torch.bfloat16)
        assert torch.equal(got, mc.bits16(want))


def test_bf16_rne_bits():
    """against torch's fp32 -> bf16 conversion on every exponent, ties of both parities, the overflow boundary and the denormals"""
    g = torch.Generator().manual_seed(2)
    u = torch.randint(-2 ** 31, 2 ** 31, (1 << 20,), generator=g, dtype=torch.int64).to(torch.int32)
    ties = (torch.arange(65536, dtype=torch.int64) << 16) | 0x8000
    ties = torch.where(ties >= 2 ** 31, ties - 2 ** 32, ties).to(torch.int32)
    f = torch.cat([u, ties, ties + 1, ties - 1]).view(torch.float32)
    f = f[~torch.isnan(f)]
    assert torch.equal(mc.bf16_rne_bits(f.double()), mc.bits16(f.to(torch.bfloat16)))
    assert mc.bf16_rne_bits(torch.tensor([2.0 ** -127, -2.0 ** -133, 2.0 ** -134, 2.0 ** 128, -1e300])).tolist() == \
        [0x0040, 0x8001, 0x0000, 0x7F80, 0xFF80]


def test_cast_and_copy_references():
    (x,), _ = mc.gen_patterns((3, 5, 7, 24), 3, 13, 17, DEV)
    f = x.float()                                       # torch's own bf16 -> fp32 conversion (NaN payloads survive the bit shift)
    assert torch.equal(mc.slice_cast(x, 3, 13), f[..., 3:16].contiguous().view(torch.int32))
    assert torch.equal(mc.nhwc_to_nchw_f32(x, 3, 13), f[..., 3:16].permute(0, 3, 1, 2).contiguous().view(torch.int32))
    (s,), _ = mc.gen_patterns((2, 4, 5, 24), 8, 16, 19, DEV)
    assert torch.equal(mc.concat_copy(s), s.view(torch.int16).to(torch.int32) & 0xFFFF)
    up = s[..., 8:24].view(torch.int16).repeat_interleave(2, 1).repeat_interleave(2, 2)
    assert torch.equal(mc.upsample2x(s, 8, 16), up.to(torch.int32) & 0xFFFF)
    b = torch.arange(65536, dtype=torch.int32)
    assert torch.equal(mc.bits16(mc.from_bits16(b)), b)
    assert torch.equal(mc.cast_bits(b), mc.from_bits16(b).float().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------------
# glue references against Python loops (bit patterns through numpy views)
# ---------------------------------------------------------------------------------------------------------------------------------
def _b(t):
    return t.contiguous().view(torch.int32).numpy()


NEG_FLT_MAX_BITS = -8388609       # 0xFF7FFFFF as int32


def test_rpn_merge_reference():
    (boxes, scores, keep), _ = mc.gen_rpn_merge([[3, 2, 7, 4], [3, 2, 7], [3, 2, 7]], 23, DEV)
    mb, ms = mc.rpn_merge(boxes, scores, keep)
    bb, sb, kb = _b(boxes), _b(scores), keep.numpy()
    for l in range(3):
        for b in range(2):
            for j in range(7):
                assert mb[b, l * 7 + j].tolist() == bb[l, b, j].tolist()
                assert int(ms[b, l * 7 + j]) == (int(sb[l, b, j]) if kb[l, b, j] != 0 else NEG_FLT_MAX_BITS)
    assert torch.tensor([NEG_FLT_MAX_BITS], dtype=torch.int32).view(torch.float32).item() == -mc.FLT_MAX


def test_make_rois_reference():
    B, P, post = 5, 9, 6
    (mboxes, topv, topi, cnt), _ = mc.gen_make_rois([[B, P, 4], [B, post], [B, post], [B]], 29, DEV)
    rois, rs = mc.make_rois(mboxes, topv, topi, cnt)
    mbb, tvb = _b(mboxes), _b(topv)
    for b in range(B):
        for j in range(post):
            e = b * post + j
            if j < int(cnt[b]):
                want, ws = [_b(torch.tensor([float(b)]))[0]] + mbb[b, int(topi[b, j])].tolist(), int(tvb[b, j])
            else:
                want, ws = [_b(torch.tensor([float(b)]))[0], 0, 0, 0, 0], 0
            assert rois[e].tolist() == want and int(rs[e]) == ws


@pytest.mark.parametrize("with_cnt", [False, True])
def test_gather_rows_reference(with_cnt):
    B, n, W, k = 5, 8, 3, 6
    (src, idx, cnt), _ = mc.gen_gather_rows([[B, n, W], [B, k]], with_cnt, 31, DEV)
    out = mc.gather_rows(src, idx, cnt)
    sb = _b(src)
    for b in range(B):
        for j in range(k):
            valid = cnt is None or j < int(cnt[b])
            assert out[b, j].tolist() == (sb[b, int(idx[b, j])].tolist() if valid else [0] * W)


@pytest.mark.parametrize("status_form", [False, True])
def test_pack_detections_reference(status_form):
    B, npre, max_det = 7, 12, 5
    for phase in range(mc.pack_phases(B)):
        ins, _ = mc.gen_pack([None, [B, npre]], max_det, status_form, 37 + phase, DEV, phase=phase)
        boxes, scores, labels, kidx, num = ins[:5]
        sel, status = (ins[5], ins[6]) if status_form else (None, None)
        d, cntv, st = mc.pack_detections(boxes, scores, labels, kidx, num, max_det, sel, status)
        bb, sb = _b(boxes), _b(scores)
        for b in range(B):
            n = min(int(num[b]), max_det)
            assert int(cntv[b]) == n
            for j in range(max_det):
                if j < n:
                    q = int(kidx[b, j])
                    want = bb[b, q].tolist() + [int(sb[b, q]), int(_b(torch.tensor([float(int(labels[b, q]))]))[0])]
                else:
                    want = [0] * 6
                assert d[b, j].tolist() == want
            if status_form:
                flag = 1 if (int(num[b]) < max_det and int(sel[b]) >= npre) else 0
                assert int(st[b]) == int(status[b]) | flag
        assert (st is None) == (not status_form)


# ---------------------------------------------------------------------------------------------------------------------------------
# the generators plant what they claim
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,k,s,p", [((2, 37, 53, 16), 3, 2, 1), ((2, 30, 31, 8), 5, 1, 2), ((1, 40, 40, 8), 5, 1, 2)])
def test_gen_pool_plants(shape, k, s, p):
    a = dict(k=k, stride=s, pad=p, zero_pad=1)
    (x,), pl = mc.gen_pool(shape, a, 41, DEV, sppf_radius=k // 2 if s == 1 else 0)
    N, H, W, C = shape
    assert not bool(torch.isnan(x.float()).any())
    assert all(pl["border"][side] > 0 for side in ("top", "bottom", "left", "right", "tl", "tr", "bl", "br")), pl["border"]
    assert bool((x[..., 0::8] < 0).all())                                  # every border window of channel 0: all taps negative
    y0 = mc.maxpool(x, k, s, p, 0)
    assert bool((y0[:, 0, :, 0] < 0).all() and (y0[:, -1, :, 0] < 0).all() and (y0[:, :, 0, 0] < 0).all() and (y0[:, :, -1, 0] < 0).all())
    assert pl["taps"] == k * k
    step, base = (k + s - 1) // s + 1, (p + s - 1) // s
    for t in range(k * k):                                                 # each planted maximum wins its own window from tap t
        assert bool((y0[:, base + (t // k) * step, base + (t % k) * step, 1] == 1024.0 + 8 * t).all())
    assert pl["plateau"] == 3 and int((x[..., 2] == 7.0).sum()) >= N * 4
    assert pl["zeros"] > 0 and bool((mc.bits16(x[..., 3]) == 0x8000).any()) and bool((mc.bits16(x[..., 3]) == 0).any())
    assert bool((x[:, H // 2:, :, 3] < 0).any())
    assert pl["infs"] > 0 and bool((x[..., 4] == float("inf")).any()) and bool((y0[..., 4] == float("-inf")).any())
    assert pl["extremes"] == 7
    if s == 1:
        assert pl["corners"] == 4
        y3 = mc.sppf(x, k)[2]
        assert float(y3[0, 0, 0, 6]) == 2048.0 and float(y3[0, H - 1, W - 1, 6]) == 2048.0 + 48
        if shape[1] == 40:                                                 # the interior maximum reaches 3R and no further
            R3, hc, wc = 3 * (k // 2), H // 2, W // 2
            assert pl["far"] == 1
            assert float(y3[0, hc, wc + R3, 6]) == 512.0 and float(y3[0, hc + R3, wc, 6]) == 512.0
            assert float(y3[0, hc, wc + R3 + 1, 6]) < 512.0 and float(y3[0, hc - R3 - 1, wc, 6]) < 512.0


def test_gen_upsample_add_plants():
    (lat, top), pl = mc.gen_upsample_add([[2, 37, 53, 16], [2, 19, 27, 16]], 43, DEV)
    assert all(pl[key] > 0 for key in ("tie_even", "tie_odd", "overflow_pos", "overflow_neg", "cancel", "subnormal")), pl
    for t in (lat, top):
        b = mc.bits16(t)
        assert bool(((b & 0x7F80) != 0).all()) and bool(((b & 0x7F80) != 0x7F80).all())     # normal numbers only
    want, sub = mc.upsample_add(lat, top)
    assert int(sub.sum()) == pl["subnormal"]
    assert int((want == 0x7F80).sum()) == pl["overflow_pos"] and int((want == 0xFF80).sum()) == pl["overflow_neg"]
    assert int((want == 0).sum()) == pl["cancel"] and not bool((want == 0x8000).any())
    assert bool(((want[sub] & 0x7F80) == 0).all()) and bool(((want[sub] & 0x7F) != 0).all())  # bf16 denormals, not flushed


def test_gen_patterns_plants():
    (x,), pl = mc.gen_patterns((2, 40, 40, 32), 8, 24, 47, DEV)
    assert pl["patterns"] == 65536 and pl["poison"] == 2 * 40 * 40 * 8
    b = mc.bits16(x)
    assert torch.unique(b[..., 8:32]).numel() == 65536
    assert bool((b[..., :8] == mc.POISON16).all())
    (x,), pl = mc.gen_patterns((1, 3, 3, 8), 0, 8, 47, DEV)
    assert 0 < pl["patterns"] <= 72 and pl["poison"] == 0
    assert mc.POISON16 != mc.SENT16 and mc.POISON32 != mc.SENT32


def test_gen_glue_plants():
    _, pl = mc.gen_rpn_merge([None, [5, 4, 300]], 53, DEV)
    assert pl["keep"] == 4 and pl["neg_zero"] > 0 and pl["neg_fltmax"] > 0
    (mboxes, topv, topi, cnt), pl = mc.gen_make_rois([[8, 50, 4], [8, 20], [8, 20], [8]], 59, DEV)
    assert sorted(set(cnt.tolist())) == [0, 1, 10, 20] and pl["counts"] == 4 and pl["first"] and pl["last"]
    past = torch.arange(20)[None, :] >= cnt[:, None]
    assert pl["poison_slots"] == int(past.sum()) > 0
    assert bool((topi[past] == 25).all()) and not bool((topi[~past] == 25).any())
    assert bool((mc.bits32(mboxes[:, 25]) == mc.POISON32).all()) and bool((mc.bits32(topv)[past] == mc.POISON32).all())
    assert bool((topi >= 0).all()) and bool((topi < 50).all())
    assert bool((topi[cnt >= 3][:, 1] == topi[cnt >= 3][:, 2]).all())          # a repeated index
    rois, rs = mc.make_rois(mboxes, topv, topi, cnt)
    assert not bool((rois == mc.POISON32).any()) and not bool((rs == mc.POISON32).any())
    (src, idx, cnt), pl = mc.gen_gather_rows([[8, 50, 4], [8, 20]], True, 61, DEV)
    assert pl["counts"] == 4 and pl["poison_slots"] > 0 and pl["first"] and pl["last"]
    assert bool((idx >= 0).all()) and bool((idx < 50).all())
    assert not bool((mc.gather_rows(src, idx, cnt) == mc.POISON32).any())
    (src, idx, cnt), pl = mc.gen_gather_rows([[8, 50, 4], [8, 20]], False, 61, DEV)
    assert cnt is None and not bool((mc.bits32(src) == mc.POISON32).any())


@pytest.mark.parametrize("B,npre,max_det", [(16, 4096, 300), (60, 2048, 100), (7, 12, 5)])
def test_gen_pack_plants(B, npre, max_det):
    combos, status, num_eq, num_above, sel_below, seen = set(), set(), 0, 0, 0, set()
    for phase in range(mc.pack_phases(B)):
        ins, pl = mc.gen_pack([None, [B, npre]], max_det, True, 67 + phase, DEV, phase=phase)
        boxes, scores, labels, kidx, num, sel, st = ins
        combos |= pl["combos"]
        status |= pl["status"]
        num_eq, num_above, sel_below = num_eq + pl["num_eq"], num_above + pl["num_above"], sel_below + pl["sel_below"]
        for n, s, w in zip(num.tolist(), sel.tolist(), st.tolist()):
            seen.add((n < max_det, s >= npre, w))
        assert bool((kidx >= 0).all()) and bool((kidx < npre).all())
        n = num.clamp(max=max_det)
        past = torch.arange(npre)[None, :] >= n[:, None]
        assert bool((kidx[past] == npre // 2).all()) and not bool((kidx[~past] == npre // 2).any())
        assert bool((mc.bits32(scores[:, npre // 2]) == mc.POISON32).all()) and bool((labels[:, npre // 2] == mc.POISON_LABEL).all())
        d, _, _ = mc.pack_detections(boxes, scores, labels, kidx, num, max_det, sel, st)
        assert not bool((d == mc.POISON32).any())
    assert combos == {(True, True), (True, False), (False, True), (False, False)}
    assert status == set(mc.STATUS_VALUES) and num_eq > 0 and num_above > 0 and sel_below > 0
    assert len(seen) == 16                     # every outcome of the condition meets every initial status word
