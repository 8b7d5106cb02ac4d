"""not gpu: the contract of md_paste_masks (tests/paste_contract.py) checked on the CPU before any device is asked.  The float64 judge
equals torch's own float64 grid_sample(bilinear, zeros, align_corners=False) on every generated case; the fp32 twin of the kernel
(oracle/np_ops.py::paste_masks) agrees with the judge on every decision outside the derived band, and on EVERY pixel in the exact regime,
equalities with the threshold included; each deliberate mistake of the judge is noticed by the same comparison."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import np_ops
from tests import paste_contract as pc

CASES = pc.small_cases()


def _twin(c):
    with np.errstate(all="ignore"):
        return np_ops.paste_masks(c.masks, c.dets, (c.H, c.W), c.thr)


@pytest.fixture(scope="module")
def twins():
    return {c.name: _twin(c) for c in CASES}


def test_case_names_are_unique_and_cover_the_lists():
    assert len({c.name for c in CASES}) == len(CASES)
    assert {(c.H, c.W) for c in CASES} == set(pc.SIZES) and {c.S for c in CASES} == set(pc.SIDES)
    thrs = {c.thr for c in CASES if not np.isnan(c.thr)}
    assert thrs == {t for t in pc.THRESHOLDS if not np.isnan(t)} and any(np.isnan(c.thr) for c in CASES)
    assert {c.kind for c in CASES} == {"free", "exact", "const_hi", "const_lo", "const_eq"}


def test_judge_equals_float64_grid_sample():
    worst, n = 0.0, 0
    for c in CASES:
        v, s, _, _ = c.judged
        d = c.dets.astype(np.float64)
        with np.errstate(all="ignore"):
            gx = (np.arange(c.W) + 0.5 - d[:, 0:1]) / (d[:, 2:3] - d[:, 0:1]) * 2.0 - 1.0           # [R, W] normalised to [-1, 1]
            gy = (np.arange(c.H) + 0.5 - d[:, 1:2]) / (d[:, 3:4] - d[:, 1:2]) * 2.0 - 1.0
        live = s.reshape(len(d), -1).any(1)
        assert np.isfinite(gx[live]).all() and np.isfinite(gy[live]).all()
        grid = np.stack(np.broadcast_arrays(np.nan_to_num(gx, nan=-9.0, posinf=9.0, neginf=-9.0)[:, None, :],
                                            np.nan_to_num(gy, nan=-9.0, posinf=9.0, neginf=-9.0)[:, :, None]), -1)
        t = F.grid_sample(torch.from_numpy(c.masks.astype(np.float64))[:, None], torch.from_numpy(np.ascontiguousarray(grid)),
                          mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0].numpy()
        if s.any():
            worst = max(worst, float(np.abs(t - v)[s].max()))
            n += int(s.sum())
    print(f"judge vs float64 grid_sample: worst |diff| {worst:.3e} over {n} in-support pixels")
    assert n > 500000 and worst <= 1e-12


def test_rows_that_paste_nothing(twins):
    for c in CASES:
        _, s, dec, _ = c.judged
        for r in c.must_be_empty:
            assert not s[r].any() and not dec[r].any() and not twins[c.name][r].any(), (c.name, r)
        if c.must_be_empty:
            assert s.any(), c.name


def test_twin_agrees_with_judge_outside_band(twins):
    for c in CASES:
        v, s, dec, free = c.judged
        bad = (twins[c.name] != dec) & ~free
        share = c.free_share()
        print(f"{c.name}: support {int(s.sum())}, free {int(free.sum())} (share {share:.2e}), twin != judge inside the band "
              f"{int(((twins[c.name] != dec) & free).sum())}")
        assert not bad.any(), (c.name, int(bad.sum()), np.argwhere(bad)[:3], v[bad][:3])
        if c.kind == "free":
            assert share <= pc.CAP, (c.name, share)
        if c.kind == "exact":
            assert not free.any()


def test_exact_regime_every_pixel_and_a_deciding_equality(twins):
    n = 0
    for c in CASES:
        if c.kind != "exact":
            continue
        v, s, dec, _ = c.judged
        np.testing.assert_array_equal(twins[c.name], dec, err_msg=c.name)
        eq = s & (v == c.thr)
        if c.thr > 0:                                    # the planted rows: the value IS the threshold, and `>=` turns the pixel on
            assert eq.any() and dec[eq].all(), c.name
            below = s & (v == np.float64(np.nextafter(np.float32(c.thr), np.float32(0))))
            assert below.any() and not dec[below].any(), c.name
        n += int(eq.sum())
    assert n > 0


def test_thresholds_at_and_below_zero_paste_the_support_and_above_one_nothing():
    for c in CASES:
        _, s, dec, _ = c.judged
        if c.thr <= 0 and c.kind == "free":
            np.testing.assert_array_equal(dec, s.astype(np.uint8), err_msg=c.name)
            assert s.any()
        if (c.thr >= 1.0 and c.kind == "free") or np.isnan(c.thr):         # 1.0 against masks below 1, 1.5, NaN
            assert not dec.any(), c.name


def test_planted_constants(twins):
    seen = set()
    for c in CASES:
        if not c.kind.startswith("const"):
            continue
        v, s, dec, free = c.judged
        inner = c.interior()
        assert inner.sum() > 100 and (inner & ~s).sum() == 0
        # (an fp32 ix within its coordinate error of 0 or S - 1 may take a border tap: those few pixels are free)
        if c.kind == "const_hi":
            assert free[inner].mean() <= pc.CAP and twins[c.name][inner & ~free].all() and dec[inner].all(), c.name
        elif c.kind == "const_lo":
            assert not free[inner].any() and not twins[c.name][inner].any() and not dec[inner].any(), c.name
        else:
            assert free[inner].all(), c.name             # all free: the band says so itself
        seen.add(c.kind)
    assert len(seen) == 3


@pytest.mark.parametrize("mistake", pc.MISTAKES)
def test_mistake_is_noticed(mistake):
    worst, flipped = 0.0, 0
    for c in CASES:
        if c.kind.startswith("const") or np.isnan(c.thr):
            continue
        v, s, dec, free = c.judged
        changed = (pc.mistaken_decisions(c.masks, c.dets, c.H, c.W, c.thr, mistake) != dec) & ~free
        if mistake == "greater":                         # flips exactly the decided equalities
            np.testing.assert_array_equal(changed, s & (v == c.thr) & ~free, err_msg=c.name)
            flipped += int(changed.sum()) if c.kind == "exact" else 0
        worst = max(worst, float(changed.sum()) / max(int(s.sum()), 1))
    print(f"{mistake}: largest share of a case's decisions changed outside the band {worst:.3f}")
    assert flipped > 0 if mistake == "greater" else worst > pc.CAP


def test_pack_and_unpack_bits():
    rng = np.random.default_rng(0)
    for W in (1, 31, 32, 33, 101):
        dec = rng.integers(0, 2, (2, 3, W)).astype(np.uint8)
        words = pc.pack_bits(dec, W)
        assert words.shape == (2, 3, (W + 31) // 32)
        bits = pc.unpack_bits(words)
        np.testing.assert_array_equal(bits[..., :W], dec)
        assert not bits[..., W:].any()
