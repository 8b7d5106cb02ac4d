"""The contract of md_paste_masks (csrc/twostage.hip), stated independently of the kernel: a float64 JUDGE of the public definition
(mmdet _do_paste_mask / torchvision paste_masks_in_image: grid_sample(bilinear, align_corners=False, zero padding) at pixel centres, then
mask >= threshold), the BAND around the threshold inside which the kernel's fp32 sequence may decide either way, the seeded case
generators, and a list of deliberate mistakes the checks must notice.  Plain numpy; used by tests/test_paste_contract_cpu.py (judge
against torch, twin against judge, mistakes) and tests/test_paste_masks_gpu.py (device against judge).

The judge does not restate the kernel's operation sequence.  Bilinear interpolation with zero padding is written as two hat-function
matrices: the weight of tap j for a sample at position p is max(0, 1 - |p - j|), so
    value[py, px] = sum_{i, j} hat(iy[py] - i) * mask[i, j] * hat(ix[px] - j),      ix = (px + 0.5 - x0) / (x1 - x0) * S - 0.5
with no floor, no fraction, no tap index and no padding logic; the inputs are taken as exact float64 numbers and nothing is rounded to
fp32.  A row with not (score > 0 and x1 > x0 and y1 > y0) is all zero.  Outside the support (ix <= -1 or ix >= S, same for y, or a
position that is not a number) the DECISION is 0 whatever the threshold: that differs from the literal grid_sample sentence only for
threshold <= 0 (where zero padding would paste the whole image) and is the operator's documented choice (include/minddet_hip.h).  A NaN
threshold or a NaN value decides 0.

CAP and the band constants below were fixed from the derivation in band() before the device was run; nothing here is tuned to it.
"""
import functools

import numpy as np

U = 2.0 ** -24          # fp32 unit roundoff
C_COORD = 8.0           # |ix_fp32 - ix| <= C_COORD * U * (|ix| + 1), derived in band()
C_VALUE = 8.0           # |v_fp32(ix_fp32, iy_fp32) - v(ix_fp32, iy_fp32)| <= C_VALUE * U * max|tap|, derived in band()
CAP = 1e-3              # largest share of a case's in-support decisions that may lie in the band

SIZES = ((1, 1), (3, 31), (5, 32), (4, 33), (7, 63), (2, 64), (9, 65), (6, 100), (5, 101), (75, 101))
SIDES = (1, 2, 7, 14, 28, 32, 56)
THRESHOLDS = (0.5, 0.25, 129.0 / 256.0, 0.0, -1.0, 1.0, 1.5, float("nan"))
MISTAKES = ("align_corners", "corners", "border", "greater", "transposed", "side_plus_one", "nearest", "scale_s_minus_1", "ceil")


# ------------------------------------------------------------------------------------------------------------------ the judge
def _positions(lo, hi, n, S, variant=None):
    p = np.arange(n, dtype=np.float64) + (0.0 if variant == "corners" else 0.5)
    side = (hi - lo) + (1.0 if variant == "side_plus_one" else 0.0)
    with np.errstate(all="ignore"):
        u = (p - lo) / side
        if variant == "align_corners":
            return u * (S - 1)
        if variant == "scale_s_minus_1":
            return u * (S - 1) - 0.5
        return u * S - 0.5


def _hat(pos, S, variant=None):
    """[n, S] interpolation weights of the S taps for each position (zero padding: taps outside [0, S) simply do not exist)"""
    j = np.arange(S, dtype=np.float64)[None, :]
    with np.errstate(all="ignore"):
        p = pos[:, None]
        if variant == "border":
            w = np.maximum(0.0, 1.0 - np.abs(np.clip(p, 0.0, S - 1.0) - j))
        elif variant == "nearest":
            w = (np.rint(p) == j).astype(np.float64)
        elif variant == "ceil":
            first = np.ceil(p)
            w = (j == first) * (1.0 - (p - first)) + (j == first + 1.0) * (p - first)
        else:
            w = np.maximum(0.0, 1.0 - np.abs(p - j))
    return np.where(np.isfinite(pos)[:, None], w, 0.0)


def _row_valid(d):
    return bool(d[4] > 0 and d[2] > d[0] and d[3] > d[1])


def _evaluate(masks, dets, H, W, variant=None):
    """-> values [R,H,W] float64 (0 outside the support), support [R,H,W] bool"""
    masks = np.asarray(masks, np.float32).astype(np.float64)
    dets = np.asarray(dets, np.float32).astype(np.float64)
    R, S = masks.shape[0], masks.shape[1]
    values, support = np.zeros((R, H, W), np.float64), np.zeros((R, H, W), bool)
    for r in range(R):
        if not _row_valid(dets[r]):
            continue
        ix = _positions(dets[r, 0], dets[r, 2], W, S, variant)
        iy = _positions(dets[r, 1], dets[r, 3], H, S, variant)
        m = masks[r].T if variant == "transposed" else masks[r]
        sup = ((iy > -1.0) & (iy < S))[:, None] & ((ix > -1.0) & (ix < S))[None, :]
        values[r] = np.where(sup, _hat(iy, S, variant) @ m @ _hat(ix, S, variant).T, 0.0)
        support[r] = sup
    return values, support


def judge_values(masks, dets, H, W):
    """[R,H,W] float64: the definition's interpolated value at every pixel centre, 0 outside the support and in invalid rows"""
    return _evaluate(masks, dets, H, W)[0]


def judge_support(masks, dets, H, W):
    return _evaluate(masks, dets, H, W)[1]


def decide(values, support, thr, strict=False):
    with np.errstate(invalid="ignore"):
        return (support & ((values > thr) if strict else (values >= thr))).astype(np.uint8)


def mistaken_decisions(masks, dets, H, W, thr, mistake):
    v, s = _evaluate(masks, dets, H, W, None if mistake == "greater" else mistake)
    return decide(v, s, thr, strict=mistake == "greater")


# ------------------------------------------------------------------------------------------------------------------ the band
def _band(masks, dets, H, W):
    masks = np.asarray(masks, np.float32).astype(np.float64)
    dets = np.asarray(dets, np.float32).astype(np.float64)
    R, S = masks.shape[0], masks.shape[1]
    bandv, edge = np.zeros((R, H, W), np.float64), np.zeros((R, H, W), bool)
    for r in range(R):
        if not _row_valid(dets[r]):
            continue
        ix, iy = _positions(dets[r, 0], dets[r, 2], W, S), _positions(dets[r, 1], dets[r, 3], H, S)
        if not (np.isfinite(ix).all() and np.isfinite(iy).all()):
            continue                                   # an infinite corner: positions are NaN (no support) or exact
        ex, ey = C_COORD * U * (np.abs(ix) + 1.0), C_COORD * U * (np.abs(iy) + 1.0)
        near_x, near_y = (ix >= -1.0 - ex) & (ix <= S + ex), (iy >= -1.0 - ey) & (iy <= S + ey)
        with np.errstate(invalid="ignore"):
            mp = np.pad(np.nan_to_num(masks[r], nan=0.0), 1)    # cells of the zero-padded mask: cell (c, d) has taps c..c+1, d..d+1
        dx, dy = np.abs(np.diff(mp, axis=1)), np.abs(np.diff(mp, axis=0))
        gx = np.maximum(dx[:-1], dx[1:])                         # largest horizontal step between the taps of a cell
        gy = np.maximum(dy[:, :-1], dy[:, 1:])
        am = np.abs(mp)
        mx = np.maximum(np.maximum(am[:-1, :-1], am[:-1, 1:]), np.maximum(am[1:, :-1], am[1:, 1:]))
        b = np.zeros((H, W), np.float64)
        for ys in (-1.0, 1.0):                                   # the cells fp32 can land in: that of ix - ex and that of ix + ex
            yc = np.clip(np.floor(iy + ys * ey) + 1, 0, S).astype(np.int64)
            for xs in (-1.0, 1.0):
                xc = np.clip(np.floor(ix + xs * ex) + 1, 0, S).astype(np.int64)
                b = np.maximum(b, (ex[None, :] * gx[yc][:, xc] + ey[:, None] * gy[yc][:, xc]) + C_VALUE * U * mx[yc][:, xc])
        near = near_y[:, None] & near_x[None, :]
        bandv[r] = np.where(near, b, 0.0)
        on_x = (np.abs(ix + 1.0) <= ex) | (np.abs(ix - S) <= ex)
        on_y = (np.abs(iy + 1.0) <= ey) | (np.abs(iy - S) <= ey)
        edge[r] = near & (on_y[:, None] | on_x[None, :])
    return bandv, edge


def band(masks, dets, H, W):
    """[R,H,W] float64: the distance from the threshold inside which the kernel's decision may go either way, per pixel.

    Derived from the kernel's documented fp32 sequence (u = 2^-24, every operation rounded on its own):
      ix_fp = fl(fl(fl(fl((px + 0.5) - x0) * fl(1 / fl(x1 - x0))) * S) - 0.5)
    px + 0.5 is exact (px < 2^15).  The subtraction, the box side, the reciprocal and the two products carry one relative rounding each:
    the value before '- 0.5' is q (1 + d), |d| <= 5u + O(u^2), q = ix + 0.5; the last subtraction adds u |ix_fp|.  So
      |ix_fp - ix| <= 5u (|ix| + 0.5) + u |ix| + O(u^2) <= 6u (|ix| + 1);           C_COORD = 8 leaves room for the second-order terms.
    The value is continuous and piecewise bilinear in (ix, iy); its slope along x is at most the largest difference of two horizontally
    neighbouring taps of the cell, the zero border included (same for y).  A coordinate error can move the sample into the next cell
    (floor(ix_fp) != floor(ix) when ix is within the error of an integer), so the largest step over the cells that ix - ex and ix + ex
    (iy - ey and iy + ey) fall into is taken: |v(ix_fp, iy_fp) - v(ix, iy)| <= ex * Gx + ey * Gy.
    At the fp32 coordinates the kernel then computes fx = ix_fp - floor (exact for ix_fp >= 0; one rounding, <= u, in (-1, 0)),
    gx = 1 - fx (<= u), and four products and three sums: each of the four weighted taps passes through two products and two sums
    (4u relative), its two weights carry up to 2u absolute each; with the weights summing to 1 that is <= 8u * max|tap| = C_VALUE.
    Together:   band = ex * Gx + ey * Gy + 8u * M,    ex = 8u (|ix| + 1),   M = largest |tap| of those cells.
    For S = 28 and values in [0, 1]: 8u * 29 + 8u * 29 + 8u = 2.8e-5 at the far corner of the mask, 1e-6 at its near one.
    Where all those taps are zero the band is zero and the fp32 value is exactly zero, as the float64 one.
    Pixels farther outside the support than the coordinate error have band 0 (both sides decide 0 there)."""
    return _band(masks, dets, H, W)[0]


def support_edge(masks, dets, H, W):
    """[R,H,W] bool: pixels whose ix (iy) lies within the coordinate error of -1 or S, where fp32 may put the pixel on the other side of
    the support's border.  There the value is within the band of 0, so this decides a pixel only when threshold <= band."""
    return _band(masks, dets, H, W)[1]


def free_pixels(values, bandv, edge, thr):
    """[R,H,W] bool: the decisions the contract leaves open (value within the band of the threshold, or a support-border pixel while the
    threshold is not above the band).  A zero band leaves nothing open: there the fp32 value equals the float64 one."""
    if np.isnan(thr):
        return np.zeros(values.shape, bool)
    with np.errstate(invalid="ignore"):
        return (bandv > 0) & ((np.abs(values - thr) <= bandv) | (edge & (thr <= bandv)))


# ------------------------------------------------------------------------------------------------------------------ the cases
class Case:
    """kind: 'free' (band and CAP apply), 'exact' (band 0, every pixel decided), 'const_hi' / 'const_lo' / 'const_eq' (planted constants,
    outside the cap)"""

    def __init__(self, name, H, W, masks, dets, thr, kind="free", must_be_empty=()):
        self.name, self.H, self.W, self.thr, self.kind = name, H, W, float(thr), kind
        self.masks = np.ascontiguousarray(masks, np.float32)
        self.dets = np.ascontiguousarray(dets, np.float32)
        self.S = self.masks.shape[1]
        self.must_be_empty = tuple(must_be_empty)       # rows that paste nothing by construction

    @functools.cached_property
    def judged(self):
        """(values, support, decisions, free) -- computed once, shared by every test that needs it, never modified"""
        v, s = _evaluate(self.masks, self.dets, self.H, self.W)
        if self.kind == "exact":
            free = np.zeros(v.shape, bool)
        else:
            free = free_pixels(v, *_band(self.masks, self.dets, self.H, self.W), self.thr)
        out = (v, s, decide(v, s, self.thr), free)
        for a in out:
            a.setflags(write=False)
        return out

    def free_share(self):
        v, s, _, free = self.judged
        return float(free.sum()) / max(int(s.sum()), 1)

    def interior(self):
        """pixels whose four taps are all in range"""
        dets = self.dets.astype(np.float64)
        out = np.zeros((len(dets), self.H, self.W), bool)
        for r in range(len(dets)):
            if _row_valid(dets[r]):
                ix, iy = _positions(dets[r, 0], dets[r, 2], self.W, self.S), _positions(dets[r, 1], dets[r, 3], self.H, self.S)
                with np.errstate(invalid="ignore"):
                    out[r] = ((iy >= 0) & (iy <= self.S - 1))[:, None] & ((ix >= 0) & (ix <= self.S - 1))[None, :]
        return out


def _dets(boxes, rng, scores=None):
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    d = np.zeros((len(boxes), 6), np.float32)
    d[:, :4] = boxes
    d[:, 4] = rng.uniform(0.05, 1.0, len(boxes)) if scores is None else scores
    d[:, 5] = rng.integers(0, 80, len(boxes))
    return d


def _loguniform_boxes(rng, H, W, n):
    bw = np.exp(rng.uniform(np.log(0.3), np.log(3.0 * W), n))
    bh = np.exp(rng.uniform(np.log(0.3), np.log(3.0 * H), n))
    cx, cy = rng.uniform(-0.1 * W, 1.1 * W, n), rng.uniform(-0.1 * H, 1.1 * H, n)
    return np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1)


def _edge_boxes(rng, H, W):
    """across each of the four image edges, and wholly outside each"""
    a, b = 0.37 * W + 0.6, 0.41 * H + 0.6
    return np.array([[-a, 0.2 * H, a, 0.9 * H + 1], [W - a, -0.3, W + a, H + 0.3], [0.1 * W, -b, 0.8 * W + 1, b], [-0.2, H - b, W + 0.7, H + b],
                     # outside by more than half a side: at S = 1 the support reaches half a side beyond the box
                     [-1.5 * a - 0.3, 0, -0.5 * a - 0.3, H], [W + 0.5 * a + 0.3, 0, W + 1.5 * a + 0.3, H],
                     [0, -1.5 * b - 0.3, W, -0.5 * b - 0.3], [0, H + 0.5 * b + 0.3, W, H + 1.5 * b + 0.3]])


def _subpixel_boxes(rng, H, W):
    """narrower than a pixel, with and without a pixel centre inside, on each axis"""
    cx, cy = float(rng.integers(0, W)), float(rng.integers(0, H))
    w_in, w_out = (cx + 0.37, cx + 0.68), (cx + 0.61, cx + 0.93)
    h_in, h_out = (cy + 0.29, cy + 0.71), (cy + 0.55, cy + 0.97)
    tall, wide = (-0.4, H + 0.3), (-0.3, W + 0.4)
    return np.array([[w_in[0], h_in[0], w_in[1], h_in[1]], [w_out[0], tall[0], w_out[1], tall[1]], [w_in[0], tall[0], w_in[1], tall[1]],
                     [wide[0], h_out[0], wide[1], h_out[1]], [wide[0], h_in[0], wide[1], h_in[1]], [w_out[0], h_out[0], w_out[1], h_out[1]]])


def _aligned_boxes(rng, H, W):
    """edges exactly on pixel centres, and exactly on pixel corners"""
    x0, y0 = float(rng.integers(0, max(W // 2, 1))), float(rng.integers(0, max(H // 2, 1)))
    x1, y1 = x0 + float(rng.integers(1, W + 3)), y0 + float(rng.integers(1, H + 3))
    return np.array([[x0 + 0.5, y0 + 0.5, x1 + 0.5, y1 + 0.5], [x0, y0, x1, y1], [x0 - 1.5, y0, x1 + 0.5, y1 + 1.0], [-1.0, -0.5, W + 1.0, H + 0.5]])


def _huge_boxes(rng, H, W):
    cx, cy = rng.uniform(0, W), rng.uniform(0, H)
    return np.array([[cx - 5e5, cy - 5e5, cx + 5e5, cy + 5e5], [cx - 5e5, 0.25 * H - 0.1, cx + 5e5, 0.75 * H + 0.6]])


def _far_boxes():
    return np.array([[32000.25, 32000.5, 32002.25, 32002.5], [-32002.0, -32001.75, -32000.0, -31999.75]])


def _degenerate_boxes(H, W):
    inf, nan = np.inf, np.nan
    return np.array([[3.0, 0.0, 3.0, H], [5.0, 0.0, 2.0, H], [0.0, 2.0, W, 2.0], [0.0, H, W, 0.0],            # x1 == x0, x1 < x0 (and y)
                     [-inf, 0.0, W, H], [0.0, 0.0, inf, H], [-inf, -inf, inf, inf], [0.0, nan, W, H], [nan, 0.0, W, H], [0.0, 0.0, W, nan]])


def _uniform_masks(rng, n, S):
    return rng.uniform(0.02, 1.0, (n, S, S))


def _blob_masks(rng, n, S):
    """sums of Gaussian blobs, peak above and tails below every tested threshold: the level set crosses the box"""
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64)
    out = np.zeros((n, S, S))
    for r in range(n):
        for _ in range(int(rng.integers(1, 4))):
            cy, cx, sg = rng.uniform(0, S), rng.uniform(0, S), rng.uniform(0.15, 0.5) * max(S, 2)
            out[r] += rng.uniform(0.6, 0.95) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg * sg))
    # overlapping blobs are scaled back under 1: a plateau of exact ones is the saturated family's business (it ties with 1/2 and 1/4
    # under boxes whose edge lies on a pixel centre, and with threshold 1 everywhere)
    return out * np.minimum(1.0, 0.97 / np.maximum(out.max(axis=(1, 2), keepdims=True), 1e-9))


def _saturated_masks(rng, n, S):
    return (_blob_masks(rng, n, S) >= 0.4).astype(np.float64)


_MASKS = (_uniform_masks, _blob_masks, _saturated_masks)


def _general_rows(rng, H, W, aligned=True):
    """boxes of every family, the rows that must paste nothing, and the scores"""
    fams = [_loguniform_boxes(rng, H, W, 8), _edge_boxes(rng, H, W), _subpixel_boxes(rng, H, W), _huge_boxes(rng, H, W)]
    if aligned:
        fams.append(_aligned_boxes(rng, H, W))
    boxes = np.concatenate(fams)
    n_live = len(boxes)
    dead = np.concatenate([_far_boxes(), _degenerate_boxes(H, W)])
    whole = np.tile(np.array([[-0.5, -0.25, W + 0.5, H + 0.25]]), (4, 1))          # valid boxes under scores 0, -0.0, -1, NaN
    all_boxes = np.concatenate([boxes, dead, whole])
    scores = np.concatenate([rng.uniform(0.05, 1.0, n_live + len(dead)), np.array([0.0, -0.0, -1.0, np.nan])])
    dets = _dets(all_boxes, rng, scores)
    # the wholly-outside edge boxes (rows 12..15), the far boxes, the degenerate ones except the two with one infinite far corner
    # (-inf .. W gives NaN positions: empty; 0 .. +inf samples at -0.5: not empty), and the four scores
    deg0 = n_live + 2
    empty = list(range(12, 16)) + [n_live, n_live + 1] + [deg0 + i for i in (0, 1, 2, 3, 4, 6, 7, 8, 9)] + list(range(len(all_boxes) - 4, len(all_boxes)))
    return dets, empty


@functools.lru_cache(maxsize=None)
def small_cases():
    """every (H, W) x S once, mask family and threshold rotating; then the special thresholds; then the exact regime and the constants"""
    cases = []
    k = 0
    for hi, (H, W) in enumerate(SIZES):
        for si, S in enumerate(SIDES):
            rng = np.random.default_rng(1000 + 10 * hi + si)
            dets, empty = _general_rows(rng, H, W)
            fam = _MASKS[k % 3]
            # 0 / 1 masks under boxes with an edge on a pixel centre give values of exactly 1/2 and 1/4 (ix = -0.5): ties with those
            # thresholds are decided, with no band, in the exact regime below; here saturated masks meet 129/256 only
            thr = THRESHOLDS[2] if fam is _saturated_masks else THRESHOLDS[(k // 3) % 3]
            k += 1
            cases.append(Case(f"{fam.__name__[1:-6]}-{H}x{W}-S{S}-t{thr:g}", H, W, fam(rng, len(dets), S), dets, thr, must_be_empty=empty))
    # thresholds 0, -1 (the support and nothing else), 1, 1.5, NaN (nothing): uniform and blob masks in (0, 1); no aligned boxes, whose
    # support border falls on pixel centres by construction (those are in the exact regime below, decided without a band)
    for ti, thr in enumerate(THRESHOLDS[3:]):
        for ci, ((H, W), S) in enumerate((((75, 101), 28), ((4, 33), 7), ((2, 64), 56), ((5, 101), 14), ((1, 1), 2))):
            rng = np.random.default_rng(2000 + 10 * ti + ci)
            dets, empty = _general_rows(rng, H, W, aligned=False)
            fam = _MASKS[ci % 2]
            cases.append(Case(f"{fam.__name__[1:-6]}-{H}x{W}-S{S}-t{thr:g}", H, W, np.maximum(fam(rng, len(dets), S), 2.0 ** -10), dets, thr,
                              must_be_empty=empty))
    cases += exact_cases() + constant_cases()
    return tuple(cases)


def _exact_boxes(rng, H, W, S, n):
    k = rng.integers(-2, 3, (n, 2))
    side = S * 2.0 ** k
    x0 = rng.integers(-4 * W, 4 * W + 1, n) / 4.0 - side[:, 0] * rng.integers(0, 2, n)
    y0 = rng.integers(-4 * H, 4 * H + 1, n) / 4.0 - side[:, 1] * rng.integers(0, 2, n)
    return np.stack([x0, y0, x0 + side[:, 0], y0 + side[:, 1]], 1)


def exact_cases():
    """S a power of two, mask values multiples of 2^-8, corners multiples of 1/4, sides S * 2^k, k in -2..2: every product and sum of the
    fp32 sequence is exact, so the twin and the device must equal the judge on EVERY pixel.  The last two rows lie under a box of side
    exactly S at integer corners: ix is an integer, the value IS a mask entry; entries equal to the threshold are planted next to
    entries one fp32 ulp lower."""
    cases = []
    n = 0
    for (H, W) in ((75, 101), (9, 65), (5, 32), (4, 33), (1, 1), (6, 100)):
        for S in (1, 2, 32):
            thr = (0.5, 0.25, 129.0 / 256.0, 1.0, 0.0, -1.0)[n % 6]
            rng = np.random.default_rng(3000 + n)
            n += 1
            R = 14
            boxes = _exact_boxes(rng, H, W, S, R)
            masks = rng.integers(0, 257, (R, S, S)).astype(np.float64) / 256.0
            masks[1] = (masks[1] >= 0.5)                                                # a saturated row
            masks[2] = (rng.integers(0, 3, (S, S)) + 127) / 256.0                        # values at and next to 0.5
            for r in (R - 2, R - 1):                                                     # the planted rows
                ox, oy = (0, 0) if r == R - 1 or S == 1 else (int(rng.integers(0, 2)), int(rng.integers(0, 2)))
                boxes[r] = (-ox, -oy, -ox + S, -oy + S)                                   # pixel (0, 0) shows entry [oy, ox]
                if thr > 0:
                    t32 = np.float32(thr)
                    lower = np.float64(np.nextafter(t32, np.float32(0)))
                    pick = rng.integers(0, 2, (S, S)).astype(bool)
                    masks[r] = np.where(pick, np.float64(t32), lower)
                    masks[r, oy, ox] = np.float64(t32) if r == R - 1 else lower
            cases.append(Case(f"exact-{H}x{W}-S{S}-t{thr:g}", H, W, masks, _dets(boxes, rng), thr, kind="exact"))
    return cases


def constant_cases():
    """masks that are the constant thr + 2^-20 (every pixel whose four taps are in range must be on), thr - 2^-20 (off) and exactly thr
    (fp32 rounds (1 - fx) + fx below 1 on some pixels: all free, the twin alone judges them)"""
    cases = []
    for ci, ((H, W), S) in enumerate((((75, 101), 28), ((5, 101), 7), ((9, 65), 56))):
        for kind, off in (("const_hi", 2.0 ** -20), ("const_lo", -2.0 ** -20), ("const_eq", 0.0)):
            rng = np.random.default_rng(4000 + ci)
            boxes = np.concatenate([_loguniform_boxes(rng, H, W, 8), _edge_boxes(rng, H, W)[:4], _aligned_boxes(rng, H, W)])
            masks = np.full((len(boxes), S, S), 0.5 + off)
            cases.append(Case(f"{kind}-{H}x{W}-S{S}", H, W, masks, _dets(boxes, rng), 0.5, kind=kind))
    return cases


def pack_bits(dec, W):
    """[R,H,W] 0/1 -> [R,H,ceil(W/32)] uint32 words, bit j of word k = pixel 32 k + j, padding bits 0"""
    R, H = dec.shape[0], dec.shape[1]
    Ww = (W + 31) // 32
    p = np.zeros((R, H, Ww * 32), np.uint64)
    p[..., :W] = dec
    return (p.reshape(R, H, Ww, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def unpack_bits(words):
    """[R,H,Ww] uint32 -> [R,H,32 Ww] uint8, the padding bits included"""
    w = words.astype(np.uint32)
    return ((w[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.uint8).reshape(*w.shape[:-1], -1)
