"""The NMS contract of tests/nms_contract.py, pinned without a GPU on every list and threshold tests/test_nms_lists_gpu.py uses:
the fp32 CPU oracle's keep lists pass the float64 judge, the inputs leave (almost) no pair undecided, each wrong greedy variant
fails the judge on the list family built to expose it, the lattice expectations are literal, and the soft-NMS reference agrees
with the published algorithm on the existing cases."""
import numpy as np
import pytest

import oracle
from oracle import np_ops
from tests import nms_contract as nc

F32 = np.float32
ALIGNED_OP = {0: "ge", 1: "gt", 2: "gt"}


# ------------------------------------------------------------------------------------------------ a plain fp32 numpy greedy
def greedy_f32(value, n, op, thr, groups=None, dead=None, quota=0, variant=None):
    """Greedy NMS in fp32 numpy; value(j, ks) = the op's fp32 quantity of box j against earlier boxes ks.  `variant` names one
    deliberate mistake."""
    t = F32(thr)
    if variant == "swap_op":
        op = {"ge": "gt", "gt": "ge", "le": "lt"}[op]
    if variant == "ignore_groups":
        groups = None
    if variant == "dead_kept":
        dead = None
    if variant in ("quota+1", "quota-1"):
        quota = quota + 1 if variant == "quota+1" else quota - 1
    keep, seen = [], []
    for j in range(n):
        if quota > 0 and len(keep) >= quota:
            break
        if dead is not None and dead[j]:
            continue
        ks = np.asarray(seen if variant == "suppressed_suppresses" else keep, np.int64)
        if variant == "lost_between_blocks" and ks.size:
            ks = ks[ks // nc.TILE != j // nc.TILE - 1]
        if groups is not None and ks.size:
            ks = ks[groups[ks] == groups[j]]
        seen.append(j)
        if ks.size:
            v = value(j, ks)
            with np.errstate(invalid="ignore"):
                hit = {"ge": v >= t, "gt": v > t, "le": v <= t, "lt": v < t}[op]
            if hit.any():
                continue
        keep.append(j)
    return np.asarray(keep, np.int64)


def aligned_value(b, mode):
    b = np.asarray(b, F32)
    return lambda j, ks: nc.aligned_ovr(b[ks], b[j], 1.0 if mode == 1 else 0.0, mode, F32)


def rot_value(b, rule):
    b = np.asarray(b, F32)
    ov, area = oracle.boxes_overlap_bev(b, b), b[:, 3] * b[:, 4]

    def value(j, ks):
        with np.errstate(all="ignore"):
            den = area[ks] + area[j] - ov[ks, j]
            return ov[ks, j] / (np.fmax(den, F32(1e-8)) if rule == "clamp" else den)
    return value


def share(und, jud):
    return und / max(jud, 1)


# ------------------------------------------------------------------------------------------------ aligned
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_aligned_oracle_keep_lists_pass_the_judge(mode):
    op = ALIGNED_OP[mode]
    und = jud = 0
    for n in nc.ALIGNED_NS:
        for thr in nc.ALIGNED_THRS:
            boxes, count, group, kinds = nc.aligned_batch(n, mode, thr, 100 * n + mode)
            for l, kind in enumerate(kinds):
                m = min(int(count[l]), n)
                keep = np.nonzero(oracle.nms_aligned(boxes[l, :m], thr, 0.0, mode, groups=group[l, :m]))[0]
                exact = kind == "lattice" and n >= 63
                band = nc.aligned_band(boxes[l], mode, exact=exact)
                u, j = nc.judge_greedy(band, m, keep, groups=group[l], op=op, thr=thr)
                np.testing.assert_array_equal(keep, greedy_f32(aligned_value(boxes[l], mode), m, op, thr, group[l]))
                if exact:
                    assert u == 0
                    np.testing.assert_array_equal(keep, nc.greedy_exact(band, m, groups=group[l], op=op, thr=thr))
                else:
                    assert share(u, j) <= 1e-3, (n, thr, kind, u, j)        # per list, and over all of them below
                    und, jud = und + u, jud + j
    for thr in nc.ALIGNED_THRS:
        boxes, group, kinds = nc.aligned_full_lists(mode, thr, 40 + mode)
        for l, kind in enumerate(kinds):
            keep = np.nonzero(oracle.nms_aligned(boxes[l], thr, 0.0, mode, groups=group[l]))[0]
            band = nc.aligned_band(boxes[l], mode, exact=kind == "lattice")
            u, j = nc.judge_greedy(band, 640, keep, groups=group[l], op=op, thr=thr)
            if kind == "chain":   # neighbours suppress, second neighbours do not: the odd indices and the lead box survive
                np.testing.assert_array_equal(keep, np.concatenate([[0], np.arange(1, 640, 2)]))
            if kind == "naninf":  # the all-NaN box suppresses nothing and nothing suppresses it, in every mode
                assert 640 // 3 in keep
                odd = np.array([640 // 4, 2 * 640 // 3, 640 // 5, 3 * 640 // 4, 640 // 2])
                if mode != 2:     # unclamped quotient: a partly NaN box and the infinite box only ever see NaN or 0
                    assert np.isin(odd, keep).all()
                    clean = boxes[l].copy()
                    clean[odd] = clean[640 // 3]        # the same list with those boxes inert: nothing else changes
                    np.testing.assert_array_equal(keep, np.nonzero(oracle.nms_aligned(clean, thr, 0.0, mode, groups=group[l]))[0])
            if kind != "lattice":
                assert share(u, j) <= 1e-3, (thr, kind, u, j)
                und, jud = und + u, jud + j
    assert jud > 20000 and share(und, jud) <= 1e-3, (und, jud)


def test_lattice_ties_separate_the_operators():
    """IoU exactly 1/2 and 1/4: `>=` (mode 0) suppresses, `>` (modes 1, 2) keeps; one step above both suppress, one below none."""
    for thr in (0.5, 0.25):
        for mode in (0, 1, 2):
            b = nc.lattice_ties(mode, thr)
            band = nc.aligned_band(b, mode, exact=True)
            keep = nc.greedy_exact(band, len(b), op=ALIGNED_OP[mode], thr=thr)
            tie_second = np.arange(1, len(b), 6)          # second box of each exact-tie pair
            above_second, below_second = tie_second + 2, tie_second + 4
            assert np.isin(tie_second, keep).all() == (mode != 0) and np.isin(tie_second, keep).any() == (mode != 0)
            assert not np.isin(above_second, keep).any() and np.isin(below_second, keep).all()
            np.testing.assert_array_equal(keep, np.nonzero(oracle.nms_aligned(b, thr, 0.0, mode))[0])
            nc.judge_greedy(band, len(b), keep, op=ALIGNED_OP[mode], thr=thr)
            for j in tie_second:                         # the planted quantity is exactly the threshold
                assert band(j, np.array([j - 1]))[0][0] == thr
        k0 = nc.greedy_exact(nc.aligned_band(nc.lattice_ties(0, thr), 0, exact=True), 24, op="ge", thr=thr)
        k2 = nc.greedy_exact(nc.aligned_band(nc.lattice_ties(2, thr), 2, exact=True), 24, op="gt", thr=thr)
        assert len(k2) - len(k0) == 4     # modes 0 and 2 differ on exactly the four tie pairs


def test_zero_area_rows_per_mode():
    """md_nms_aligned has no dead-area rule; what four coincident zero-extent boxes do follows from each mode's formula: mode 0 with
    eps 0 sees 0/0 = NaN and mode 2 sees 0 / 1e-8 = 0 (all kept), mode 1 gives each an area of one pixel and ovr 1 (first kept)."""
    z = np.zeros((4, 4), F32)
    for mode, want in nc.ZERO_ROWS_KEPT.items():
        assert np.nonzero(oracle.nms_aligned(z, 0.5, 0.0, mode))[0].tolist() == want
        keep = greedy_f32(aligned_value(z, mode), 4, ALIGNED_OP[mode], 0.5)
        assert keep.tolist() == want
        nc.judge_greedy(nc.aligned_band(z, mode, exact=True), 4, keep, op=ALIGNED_OP[mode], thr=0.5)
    assert np.nonzero(oracle.nms_aligned(z, 0.5, 1.0, 0))[0].tolist() == [0]      # mode 0 with eps 1: area 1 each, as mode 1


def test_lattice_expectations_literal():
    b = F32([[0, 0, 20, 7], [0, 0, 10, 7], [0, 0, 11, 7], [100, 0, 120, 7], [0, 0, 21, 7], [100, 0, 110, 7]])
    # modes 0, 2: box 1 vs 0 is exactly 1/2, 2 vs 0 is 11/20, 4 vs 0 is 20/21, 5 vs 3 is exactly 1/2: `>=` drops the ties, `>` keeps
    # them.  mode 1 (+1 pixel): 1 vs 0 is 88/168 and 5 vs 3 likewise, above 1/2
    exp = {0: [0, 3], 1: [0, 3], 2: [0, 1, 3, 5]}
    for mode in (0, 1, 2):
        keep = nc.greedy_exact(nc.aligned_band(b, mode, exact=True), 6, op=ALIGNED_OP[mode], thr=0.5)
        assert keep.tolist() == exp[mode], (mode, keep)
    # class keys: boxes 1, 2, 5 are of another class than 0, 3, 4
    g = np.array([0, 1, 1, 0, 0, 1], np.int32)
    keep = nc.greedy_exact(nc.aligned_band(b, 2, exact=True), 6, groups=g, op="gt", thr=0.5)
    assert keep.tolist() == [0, 1, 3, 5]        # 2 dropped by 1 (10/11), 4 by 0 (20/21), 5 kept: box 3 is of the other class
    # quota 2 cuts after the second kept box; a dead box is never kept
    assert nc.greedy_exact(nc.aligned_band(b, 2, exact=True), 6, quota=2, op="gt", thr=0.5).tolist() == [0, 1]
    dead = np.array([1, 0, 0, 0, 0, 0], bool)    # without box 0: 4 vs 1 is 70/147, kept
    assert nc.greedy_exact(nc.aligned_band(b, 2, exact=True), 6, dead=dead, op="gt", thr=0.5).tolist() == [1, 3, 4, 5]
    # circle: squared distance exactly thresh suppresses (<=); at thresh 24 box 1 survives and drops box 3 (4 + 9)
    xy = F32([[0, 0], [3, 4], [6, 8], [5, 1], [30, 30]])
    assert nc.greedy_exact(nc.circle_band(xy, exact=True), 5, op="le", thr=25.0).tolist() == [0, 2, 3, 4]
    assert nc.greedy_exact(nc.circle_band(xy, exact=True), 5, op="le", thr=24.0).tolist() == [0, 1, 2, 4]


@pytest.mark.parametrize("quota", [1, 63, 64, 65])
def test_quota_lists_pass_the_judge(quota):
    for mode in (0, 1, 2):
        boxes, _, group, kinds = nc.aligned_batch(640, mode, 0.5, 900 + quota)
        # survivors exactly the quota, and one survivor short: quota (resp. quota - 1) cells, every later box a copy
        rng = np.random.default_rng(quota)
        full = np.concatenate([np.arange(quota), rng.integers(0, quota, 640 - quota)])
        short = np.concatenate([np.arange(quota - 1), rng.integers(0, max(quota - 1, 1), 640 - quota + 1)])[:640]
        lists = [(boxes[l], group[l]) for l in range(4)] + [(nc.slot_aligned(p, quota + i), np.zeros(640, np.int32)) for i, p in enumerate((full, short))]
        for i, (b, g) in enumerate(lists):
            keep = greedy_f32(aligned_value(b, mode), 640, ALIGNED_OP[mode], 0.5, g, quota=quota)
            nc.judge_greedy(nc.aligned_band(b, mode), 640, keep, groups=g, quota=quota, op=ALIGNED_OP[mode], thr=0.5)
            if i == 4:
                assert len(keep) == quota and keep[-1] == quota - 1
            if i == 5 and quota > 1:
                assert len(keep) == quota - 1


@pytest.mark.parametrize("quota,n", [(100, 1023), (100, 1024), (100, 1100), (300, 2431), (300, 2432), (300, 2500)])
def test_quota_prefix_batch_has_the_planted_structure(quota, n):
    boxes, count, group, P = nc.quota_prefix_batch(n, quota, quota + n)
    assert P == {100: 512, 300: 1216}[quota]
    kept = []
    for l in range(6):
        m = min(int(count[l]), n)
        keep = greedy_f32(aligned_value(boxes[l], 2), m, "gt", 0.5, group[l], quota=quota)
        u, j = nc.judge_greedy(nc.aligned_band(boxes[l], 2), m, keep, groups=group[l], quota=quota, op="gt", thr=0.5)
        assert u == 0
        kept.append(keep)
    assert len(kept[0]) == quota and kept[0][-1] == P - 1                    # fills the quota at box P-1
    assert len(kept[1]) == quota and kept[1][-1] == P                        # needs box P
    assert (kept[2] < P).sum() == 3 and len(kept[2]) == min(quota, 3 + max(n - P - 90, 0))   # the prefix collapses
    assert count[3] < P and count[5] == 0 and len(kept[5]) == 0


def test_rank_cap_lists_keep_every_first_copy():
    b4, xy, b7 = nc.rank_cap_lists()
    n = len(b4)
    want = np.arange(4288)
    for band, op, thr in [(nc.aligned_band(b4, 2, exact=True), "gt", 0.5), (nc.circle_band(xy, exact=True), "le", 4.0)]:
        np.testing.assert_array_equal(nc.greedy_exact(band, n, op=op, thr=thr), want)
    np.testing.assert_array_equal(greedy_f32(lambda j, ks: nc.normal_iou(b7[ks], b7[j], F32), n, "gt", 0.5), want)
    nc.judge_greedy(nc.normal_band(b7), n, want, op="gt", thr=0.5)
    assert n == 4416 and want[-1] >= nc.SCAN_KEEP_CAP + 128


# ------------------------------------------------------------------------------------------------ normal, circle
def test_normal_and_circle_oracle_keep_lists_pass_the_judge():
    und = jud = 0
    for name, (b, thr, exact) in nc.normal_lists().items():
        keep, num = oracle.nms_normal_mask(b, thr)
        u, j = nc.judge_greedy(nc.normal_band(b), len(b), keep[:num], op="gt", thr=thr)
        if exact:   # the tie pairs are undecided for the band; the expectation is literal: tie kept (>), above dropped, below kept
            sec = np.arange(1, len(b), 6)
            assert np.isin(sec, keep[:num]).all() and not np.isin(sec + 2, keep[:num]).any() and np.isin(sec + 4, keep[:num]).all()
            assert u == len(sec)
        else:
            assert share(u, j) <= 1e-3, (name, u, j)
            und, jud = und + u, jud + j
        if name.startswith("chain"):
            np.testing.assert_array_equal(keep[:num], np.concatenate([[0], np.arange(1, len(b), 2)]))
        if name.startswith("nan"):
            # fmaxf / fminf and the clamped union: the NaN boxes take part.  The all-NaN row and the NaN-yaw row aside, each is
            # dropped or drops something: the list differs from the one with those rows far away
            n = len(b)
            away = b.copy()
            away[[n // 5, n // 3, n // 2]] = [1e4, 1e4, 0, 1, 1, 1, 0]
            k2, n2 = oracle.nms_normal_mask(away, thr)
            assert not np.array_equal(keep[:num], k2[:n2])
            big = nc.normal_iou(b[: n // 2], b[n // 2], F32)           # NaN dx: the union clamps to 1e-8
            assert ((big == 0) | (big > 1e6)).all() and (big > 1e6).any()
    assert jud > 5000 and share(und, jud) <= 1e-3, (und, jud)
    und = jud = 0
    for name, (xy, thr, exact) in nc.circle_lists().items():
        d = np.concatenate([xy, np.zeros((len(xy), 1), F32)], 1)
        keep = np.nonzero(oracle.circle_nms(d, thr))[0]
        band = nc.circle_band(xy, exact=exact)
        u, j = nc.judge_greedy(band, len(xy), keep, op="le", thr=thr)
        if exact:
            assert u == 0
            np.testing.assert_array_equal(keep, nc.greedy_exact(band, len(xy), op="le", thr=thr))
            for q in range(4):      # squared distance exactly 25: dropped; 26: kept; 20 (the last two): dropped
                assert 8 * q + 65 not in keep and band(8 * q + 65, np.array([8 * q]))[0][0] == 25.0
            assert 8 * 4 + 65 in keep and 8 * 5 + 65 in keep and 8 * 6 + 65 not in keep
        else:
            assert share(u, j) <= 1e-3, (name, u, j)
            und, jud = und + u, jud + j
        if name.startswith("chain"):
            np.testing.assert_array_equal(keep, np.concatenate([[0], np.arange(1, len(xy), 2)]))
    assert jud > 5000 and share(und, jud) <= 1e-3, (und, jud)


# ------------------------------------------------------------------------------------------------ rotated
@pytest.fixture(scope="module")
def rot_lists():
    """name -> (boxes, thr, geometry-only overlap band matrices)"""
    return {k: (b, thr, nc.rot_overlap_matrix(b, b)) for k, (b, thr) in nc.rot_lists().items()}


def test_rotated_slack_is_the_measured_one_times_four(rot_lists):
    worst = 0.0
    for name, (b, thr, ov) in rot_lists.items():
        lo, hi = ov
        o = oracle.boxes_overlap_bev(b, b).astype(np.float64)
        worst = max(worst, float((np.maximum(np.maximum(lo - o, o - hi), 0) / (1 + hi)).max()))
    print(f"largest excursion of the fp32 oracle outside the geometric band: {worst:.3e} (recorded {nc.ROT_SLACK_MEASURED:.3e})")
    # the recorded figure is bracketed loosely (it moves with the host's libm); the bands' own slack is what must hold
    assert worst <= nc.ROT_SLACK and nc.ROT_SLACK == 4 * nc.ROT_SLACK_MEASURED
    assert 0.25 * nc.ROT_SLACK_MEASURED <= worst <= 2 * nc.ROT_SLACK_MEASURED


def test_rotated_oracle_keep_lists_pass_the_judge(rot_lists):
    for name, (b, thr, ov) in rot_lists.items():
        n = len(b)
        for rule, fn, op in (("clamp", oracle.nms_rot_mask, "gt"), ("none", oracle.nms_rot_aot, "ge")):
            keep, num = fn(b, thr)
            dead = nc.rot_dead(b) if rule == "none" else None
            u, j = nc.judge_greedy(nc.rot_band(b, rule, ov), n, keep[:num], dead=dead, op=op, thr=thr)
            np.testing.assert_array_equal(keep[:num], greedy_f32(rot_value(b, rule), n, op, thr, dead=dead))
            if name.startswith("dead-only"):
                # zero-area boxes: boxes_iou_nms_gpu keeps none; NmsGpu's IoU is overlap / 1e-8 with an overlap anywhere in
                # [0, 0.04] -- the geometry cannot decide those pairs and the share condition does not apply
                assert num == 0 if rule == "none" else num > 0
                continue
            if name.startswith("nested"):    # three planted exact ties, asserted literally in the test below
                assert u == 3
                continue
            if name.startswith("nan"):       # overlap 0 against everything: the NaN rows are kept and drop nothing
                assert np.isin([n // 5, n // 3, n // 2, n // 4], keep[:num]).all()
            assert share(u, j) <= 0.02, (name, rule, u, j)
            if name.startswith("chain"):
                np.testing.assert_array_equal(keep[:num], np.concatenate([[0], np.arange(1, n, 2)]))
            if name.startswith("tail") and rule == "clamp":
                assert np.isin(np.arange(n - 21, n), keep[:num]).all()    # zero rows: IoU 0 / 1e-8 = 0 among themselves, all kept
            if name.startswith("tail") and rule == "none":
                assert not np.isin(np.arange(n - 21, n), keep[:num]).any()   # ... and dead for boxes_iou_nms_gpu


def test_rotated_nested_ties_separate_the_operators():
    """Overlap / union exactly thr: NmsGpu (>) keeps the inner box, boxes_iou_nms_gpu (>=) drops it; the geometric band cannot
    decide these pairs, the expectation is literal."""
    for thr in (0.5, 0.25):
        b = nc.rot_nested_ties(thr)
        sec = np.arange(1, len(b), 6)
        assert (oracle.boxes_iou_bev(b, b)[sec - 1, sec] == F32(thr)).all()
        for fn, tie_kept in ((oracle.nms_rot_mask, True), (oracle.nms_rot_aot, False)):
            keep, num = fn(b, thr)
            keep = keep[:num]
            assert np.isin(sec, keep).all() == tie_kept and np.isin(sec, keep).any() == tie_kept
            assert not np.isin(sec + 2, keep).any() and np.isin(sec + 4, keep).all() and np.isin(np.arange(0, len(b), 2), keep).all()


# ------------------------------------------------------------------------------------------------ wrong variants
def _fails(band, n, keep, **kw):
    try:
        nc.judge_greedy(band, n, keep, **kw)
    except nc.ContractViolation:
        return True
    return False


def test_each_wrong_variant_fails_the_judge(rot_lists):
    caught = {}

    def run(family, variants, band, value, n, op, thr, groups=None, dead=None, quota=0):
        if isinstance(variants, str):
            variants = (variants,)
        kw = dict(groups=groups, dead=dead, quota=quota, op=op, thr=thr)
        assert not _fails(band, n, greedy_f32(value, n, op, thr, groups, dead, quota), **kw)
        for variant in variants:
            if _fails(band, n, greedy_f32(value, n, op, thr, groups, dead, quota, variant=variant), **kw):
                caught.setdefault(variant, set()).add(family)

    for mode in (0, 1, 2):
        op = ALIGNED_OP[mode]
        for thr in (0.5, 0.25):
            t = nc.lattice_ties(mode, thr)
            run(f"ties-mode{mode}", "swap_op", nc.aligned_band(t, mode, exact=True), aligned_value(t, mode), len(t), op, thr)
        boxes, group, kinds = nc.aligned_full_lists(mode, 0.5, 40 + mode)
        for l, kind in enumerate(kinds):
            band, value = nc.aligned_band(boxes[l], mode, exact=kind == "lattice"), aligned_value(boxes[l], mode)
            run(kind, ("ignore_groups", "suppressed_suppresses", "lost_between_blocks"), band, value, 640, op, 0.5, group[l])
            run(kind, ("quota+1", "quota-1"), band, value, 640, op, 0.5, group[l], quota=64)
    xy, thr, _ = nc.circle_lists()["lattice"]
    run("circle-lattice", "swap_op", nc.circle_band(xy, exact=True), lambda j, ks: nc.circle_d2(xy[ks], xy[j], F32), len(xy), "le", thr)
    for name, (b, thr, ov) in rot_lists.items():
        if name.startswith("dead-only") or len(b) > 65:      # the 65-box lists have the tile boundary this needs
            continue
        fam = "rot-" + name.split("-")[0]
        run(fam, ("suppressed_suppresses", "lost_between_blocks"), nc.rot_band(b, "clamp", ov), rot_value(b, "clamp"), len(b), "gt", thr)
        run(fam, "dead_kept", nc.rot_band(b, "none", ov), rot_value(b, "none"), len(b), "ge", thr, dead=nc.rot_dead(b))
    print({k: sorted(v) for k, v in caught.items()})
    # `>` for `>=` (mode 0), `>=` for `>` (modes 1, 2) and `<` for `<=` (circle), each on its exact ties
    assert {"ties-mode0", "ties-mode1", "ties-mode2", "circle-lattice"} <= caught["swap_op"]
    assert "clustered80" in caught["ignore_groups"]
    assert {"chain", "rot-chain"} <= caught["suppressed_suppresses"]
    assert {"chain", "clustered80", "rot-chain"} <= caught["lost_between_blocks"]
    assert "rot-tail" in caught["dead_kept"]
    assert caught["quota+1"] and caught["quota-1"]


# ------------------------------------------------------------------------------------------------ soft-NMS
def test_soft_reference_agrees_with_the_published_algorithm_on_the_existing_cases():
    """The inputs of tests/test_detops_gpu.py::test_soft_nms_vs_published_algorithm: same survivors as np_ops.soft_nms, scores within
    the derived bound, and the derived bound is not looser there than that test's 2e-6 * max(1, |s|)."""
    rng = np.random.default_rng(2)
    for n, method in [(100, 2), (37, 2), (100, 1), (1, 2), (300, 2)]:
        cx, cy = rng.uniform(0, 200, n), rng.uniform(0, 150, n)
        w, h = rng.uniform(10, 80, n), rng.uniform(10, 80, n)
        boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(F32)
        scores = (rng.uniform(0.01, 1, n) + np.arange(n) * 1e-6).astype(F32)
        ref = nc.soft_nms_ref(boxes, scores, n, method=method)
        tagged = np.concatenate([boxes, scores[:, None], np.arange(n, dtype=F32)[:, None]], 1).astype(F32)
        cnt = np_ops.soft_nms(tagged, method=method)
        surv = {int(r[5]): float(r[4]) for r in tagged[:cnt]}
        tol = nc.soft_tolerance(ref)
        assert set(surv) == set(ref["order"].tolist()) == set(np.nonzero(ref["scores"] > 0)[0].tolist())
        for i, s in surv.items():
            assert abs(s - ref["scores"][i]) <= tol[i], (i, s, ref["scores"][i], tol[i])
            assert tol[i] <= 2e-6 * max(1.0, abs(s)) + 1e-12


def test_soft_cases_meet_the_planted_conditions():
    for n, method, seed, ties, threshold in nc.soft_cases():
        boxes, scores, ref = nc.soft_nms_case(n, method, seed, ties, threshold)
        assert ref["violations"] == 0 and len(set(ref["order"].tolist())) == len(ref["order"])
        sel = ref["order"]
        if ties:
            s = ref["scores"][sel]
            tie = np.nonzero((s[1:] == s[:-1]) & (ref["ndecay"][sel][1:] == 0) & (ref["ndecay"][sel][:-1] == 0))[0]
            assert len(tie) == ties // 2 and (sel[tie] < sel[tie + 1]).all()      # exact ties, decided by the lower index
        if n >= 64:   # the lists decay and drop: most boxes are decayed, some fall below the threshold
            assert (ref["ndecay"] > 0).sum() > n // 4
            assert (ref["scores"] == 0).sum() > 0 or (method != 3 and threshold < 0.01)
