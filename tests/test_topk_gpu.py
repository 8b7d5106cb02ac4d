"""-m gpu: md_topk_segmented on every form it can launch, at the sizes and with the data the detectors feed it, compared EXACTLY
(indices, values, counts and the padding) with np_ops.topk_desc_stable: NumPy's stable argsort, values taken as exact.

The forms (md_topk_last_path reports which one a call launched; every case asserts the one it meant to reach):
  A   multi-workgroup (max_segment > 32768, L <= 65535): a histogram of the top 11 bits of the order-preserving key, a compaction
      of the candidates (bin >= b1, the bin of the k-th score) and one sort of at most 8192 candidates.  The sort form follows
      the candidate count nc: <= 1024, <= 2048, <= 4096, <= 8192.
  A'  the same launch when nc > 8192 (bunched or tied top scores), or a segment longer than max_segment: the single-workgroup
      select over global memory.  nc is computed here with the kernel's own rule (path_a_candidates) to prove the band.
  B   LDS-staged (1 <= max_segment <= 30000); B' the same launch for a segment longer than the declared max_segment.
  C   one workgroup per segment (max_segment 0 = unknown, 30000 < max_segment <= 32768, or more than 65535 segments).
Inside the single-workgroup select: take-all (k >= avail), the k-th value's copies taken unordered (exactly the missing number
exist) or by an ordered index scan (more exist), and bitonic sorts for P <= 1024, 2048 and 4096 keys.

Semantics pinned: descending, ties to the lower index (relative to the segment), only scores > min_score selectable, count =
min(k, #selectable), padding (-FLT_MAX, 0) past count; -0.0 and +0.0 are one value (returned as +0.0).  NaN scores have no
specified order and are not tested."""
import numpy as np
import pytest
import torch

from oracle import np_ops
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
FLT_MAX = np.float32(3.4028234663852886e38)
PATH_C, PATH_B, PATH_A = 1, 2, 3
KS = (1, 1024, 1025, 2048, 2049, 4096)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bf16_logits(rng, n, scale=1.0, loc=0.0):
    """RPN-like objectness logits: the conv head's bf16 output, widened to fp32 (graphs.py RPN select)."""
    return (torch.from_numpy(rng.normal(loc, scale, n).astype(np.float32)).to(torch.bfloat16).float().numpy())


def ford(x):
    """The kernels' order-preserving uint32 key (-0.0 folded onto +0.0)."""
    u = np.asarray(x, np.float32).reshape(-1).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def path_a_candidates(seg, k, min_score):
    """Path A's candidate count, by the kernel's rule: b1 = the largest 11-bit bin b with count(bins >= b) >= k (0 if fewer than k
    scores are selectable); nc = #{selectable : key >> 21 >= b1}."""
    key = ford(seg)
    bins = key[key > ford(np.float32(min_score))[0]] >> 21
    suf = np.cumsum(np.bincount(bins, minlength=2048)[::-1])[::-1]
    ok = np.flatnonzero(suf >= k)
    b1 = ok.max() if ok.size else 0
    return int((bins >= b1).sum())


def band(nc):
    """topk_final_kernel's sort form for nc candidates; 'A-prime' = the overflow fallback"""
    return "<=1024" if nc <= 1024 else "<=2048" if nc <= 2048 else "<=4096" if nc <= 4096 else "<=8192" if nc <= 8192 else "A-prime"


def last_path():
    from minddet_amd import _lib

    return _lib.lib().md_topk_last_path()


def ref_topk(seg, k, min_score):
    sel = seg > np.float32(min_score)
    rv, ri = np_ops.topk_desc_stable(np.where(sel, seg, -np.inf).astype(np.float32), k)
    m = min(k, int(sel.sum()))
    return rv[:m], ri[:m], m


def run(segs, k, min_score=None, max_segment=None, path=None):
    """Top-k over the ragged list `segs`; checks the form launched and every segment against the reference.  Returns (v, i, c)."""
    from minddet_amd import det_ops

    lens = [len(s) for s in segs]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    flat = np.concatenate([np.asarray(s, np.float32) for s in segs]) if off[-1] else np.zeros(0, np.float32)
    v, i, c = det_ops.topk_segmented(T(flat), T(off), k, min_score=min_score,
                                     max_segment=max(lens) if max_segment is None else max_segment)
    got_path = last_path()
    v, i, c = v.cpu().numpy(), i.cpu().numpy(), c.cpu().numpy()
    if path is not None:
        assert got_path == path, (got_path, path)
    ms = -FLT_MAX if min_score is None else np.float32(min_score)
    for l, seg in enumerate(segs):
        rv, ri, m = ref_topk(np.asarray(seg, np.float32), k, ms)
        assert c[l] == m, (l, c[l], m)
        np.testing.assert_array_equal(i[l, :m], ri, err_msg=f"segment {l} (n {lens[l]}, k {k}): indices")
        # bit-exact values; a -0.0 input comes back as +0.0 (the same value)
        np.testing.assert_array_equal(v[l, :m].view(np.uint32), (rv + np.float32(0)).view(np.uint32), err_msg=f"segment {l}: values")
        assert (v[l, m:] == -FLT_MAX).all() and (i[l, m:] == 0).all(), f"segment {l}: padding"
    return v, i, c


def banded(n, k, nc, rng, k_hi=None):
    """A segment of n scores whose path-A candidate count is exactly nc (nc >= k): k_hi (< k) scores in bins above [1, 1.25),
    nc - k_hi scores in the single bin [1, 1.25) (so the k-th score's bin), the rest below it; shuffled."""
    k_hi = k - 1 if k_hi is None else k_hi
    s = np.concatenate([rng.uniform(2.0, 64.0, k_hi), rng.uniform(1.0, 1.2499, nc - k_hi), rng.uniform(0.01, 0.99, n - nc)])
    return rng.permutation(s.astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ path A / A'
def test_path_a_rpn_bf16_logits_production_sizes():
    """RPN P2 / P3 (201 600 / 50 400 anchors per image, batch 2, k 1000) on bf16-valued logits; R-CNN candidates (80 000, k 2048,
    min_score 0.05).  Reports where realistic data lands among the candidate bands."""
    rng = np.random.default_rng(0)
    report = {}
    for n, k, ms, mk in [(201600, 1000, None, lambda: bf16_logits(rng, 201600, 2.0, -4.0)),
                         (50400, 1000, None, lambda: bf16_logits(rng, 50400, 2.0, -4.0)),
                         (80000, 2048, 0.05, lambda: rng.beta(0.3, 6.0, 80000).astype(np.float32))]:
        segs = [mk(), mk()]
        report[(n, k)] = [band(path_a_candidates(s, k, -FLT_MAX if ms is None else ms)) for s in segs]
        run(segs, k, min_score=ms, max_segment=n, path=PATH_A)
    print("path-A candidate bands of realistic data:", report)


@pytest.mark.parametrize("k", KS)
def test_path_a_every_sort_form_and_k_edge(k):
    """201 600-score segments built so nc lands in each of topk_final's four sort forms and in the overflow fallback, at every k
    edge; a ragged list with segments of length 0 and 1 rides along (fewer than k selectable: everything is a candidate)."""
    rng = np.random.default_rng(k)
    n = 201600
    segs, want = [], []
    for nc in sorted({max(k, 700), max(k, 1500), max(k, 3000), max(k, 6000), 8192, 8193, 12000}):
        if nc < k:
            continue
        segs.append(banded(n, k, nc, rng))
        want.append(band(nc))
        assert band(path_a_candidates(segs[-1], k, -FLT_MAX)) == want[-1] and path_a_candidates(segs[-1], k, -FLT_MAX) == nc
    segs += [np.zeros(0, np.float32), np.float32([0.5]), rng.uniform(0, 1, 40000).astype(np.float32)]
    run(segs, k, max_segment=n, path=PATH_A)
    assert "A-prime" in want and (k > 1024 or "<=1024" in want) and "<=8192" in want


def test_path_a_overflow_on_ties_and_narrow_bf16():
    """A': every score the same (201 600 copies: the k-th value's ties taken by index), a long plateau at the k-th value, and bf16
    logits with a narrow spread (a handful of distinct values) -- all with nc > 8192; k edges inside the fallback's select."""
    rng = np.random.default_rng(5)
    n = 201600
    same = np.full(n, 0.25, np.float32)
    narrow = bf16_logits(rng, n, 0.02, 1.0)
    for k in KS:
        plateau = rng.uniform(0, 0.5, n).astype(np.float32)
        pos = rng.permutation(n)
        plateau[pos[:k - 1]] = rng.uniform(0.75, 1.0, k - 1)
        plateau[pos[k - 1:k + 19999]] = 0.625                   # the k-th value, 20 000 copies
        for s in (same, plateau, narrow):
            assert path_a_candidates(s, k, -FLT_MAX) > 8192
        run([same, plateau, narrow], k, max_segment=n, path=PATH_A)


def test_path_a_exact_tie_counts_and_avail_edges():
    """k == avail and k == avail + 1 (min_score decides avail), and a k-th value with exactly the missing number of copies next to one
    with more, on the candidate path and on its overflow fallback"""
    rng = np.random.default_rng(7)
    n, k = 60000, 1025
    base = rng.uniform(0.0, 0.5, n).astype(np.float32)
    for avail in (k, k - 1):
        s = base.copy()
        s[rng.choice(n, avail, replace=False)] = rng.uniform(0.6, 1.0, avail).astype(np.float32)
        run([s, s[::-1].copy()], k, min_score=0.5, max_segment=n, path=PATH_A)
    segs = []
    for copies, more, same_bin in [(3, 0, 0), (3, 9000, 0), (3, 0, 9000)]:
        s = base.copy()
        pos = rng.permutation(n)
        s[pos[:k - copies]] = rng.uniform(0.8, 1.0, k - copies).astype(np.float32)
        s[pos[k - copies:k]] = 0.7                                  # exactly the missing copies ...
        s[pos[k:k + more]] = 0.7                                    # ... or 9000 more (nc > 8192: A', ordered tie scan)
        s[pos[k + more:k + more + same_bin]] = rng.uniform(0.626, 0.69, same_bin)   # A' with the unordered take: the bin, not the value, is crowded
        assert band(path_a_candidates(s, k, -FLT_MAX)) == ("<=2048" if more + same_bin == 0 else "A-prime")
        segs.append(s)
    run(segs, k, max_segment=n, path=PATH_A)


def test_path_a_segment_longer_than_max_segment():
    """A segment longer than the declared max_segment: the chunk grid of the histogram / compaction covers only max_segment scores,
    so the segment must take the single-workgroup fallback (it used to lose its tail silently)."""
    rng = np.random.default_rng(8)
    long_ = rng.uniform(0, 1, 100000).astype(np.float32)
    long_[90000:90010] = 2.0            # the best scores sit past the first 40 000
    short = rng.uniform(0, 1, 30000).astype(np.float32)
    run([short, long_], 1000, max_segment=40000, path=PATH_A)


def test_path_a_is_deterministic():
    """The histogram and the candidate compaction use atomics (the candidates land in a different order each run); the result must
    not depend on it."""
    from minddet_amd import det_ops

    rng = np.random.default_rng(9)
    s = np.concatenate([bf16_logits(rng, 201600, 1.5), bf16_logits(rng, 201600, 0.03)])
    off = T(np.int32([0, 201600, 403200]))
    a = [x.cpu().numpy() for x in det_ops.topk_segmented(T(s), off, 2049, max_segment=201600)]
    assert last_path() == PATH_A
    b = [x.cpu().numpy() for x in det_ops.topk_segmented(T(s), off, 2049, max_segment=201600)]
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ path B / B'
def test_path_b_yolo_and_centerpoint_data():
    """YOLOv5s / YOLOv8 (25 200 / 8 400 per image, k 4096, mostly -FLT_MAX with a few thousand live scores), (8 400, 300),
    (30 000, 1000), CenterPoint (16 384, k 1000, mostly -1 with fewer than k positives: the -1 ties are taken by index)."""
    rng = np.random.default_rng(10)

    def yolo(n, live):
        s = np.full(n, -FLT_MAX, np.float32)
        s[rng.choice(n, live, replace=False)] = np.round(rng.uniform(0.001, 1, live) * 256) / 256   # bf16-ish: ties
        return s

    run([yolo(25200, 3000), yolo(25200, 5000), yolo(25200, 0)], 4096, path=PATH_B)
    run([yolo(8400, 2500), yolo(8400, 8400)], 4096, path=PATH_B)
    run([yolo(8400, 2500), yolo(8400, 200)], 300, path=PATH_B)
    run([bf16_logits(rng, 30000), rng.uniform(0, 1, 30000).astype(np.float32)], 1000, path=PATH_B)
    cp = np.full((2, 16384), -1.0, np.float32)
    cp[0, rng.choice(16384, 600, replace=False)] = rng.uniform(0.1, 1, 600)
    cp[1, rng.choice(16384, 40, replace=False)] = 0.5
    run([cp[0], cp[1]], 1000, path=PATH_B)
    run([cp[0], cp[1]], 1000, min_score=-1.0, path=PATH_B)       # the -1 are not selectable: count = #positives


@pytest.mark.parametrize("k", KS)
def test_path_b_every_sort_form_and_tie_branch(k):
    """Per k edge: all-equal segments (30 000 copies: the ordered tie scan), a k-th value with exactly the missing number of copies
    (the unordered take) next to one with more, k == avail and avail + 1 (take-all), and lengths 0 and 1, in one ragged list."""
    rng = np.random.default_rng(100 + k)
    n = 30000
    segs = [np.full(n, 0.5, np.float32), np.zeros(0, np.float32), np.float32([-3.0])]
    for copies, extra in [(3, 0), (3, 50), (700, 0), (700, 2000)]:
        c = min(copies, k)
        s = rng.uniform(0, 0.4, n).astype(np.float32)
        pos = rng.permutation(n)
        s[pos[:k - c]] = rng.uniform(0.5, 1, k - c)
        s[pos[k - c:k + extra]] = 0.45
        segs.append(s)
    for avail in (k, k - 1):
        s = np.full(n // 2, -FLT_MAX, np.float32)
        s[rng.choice(n // 2, avail, replace=False)] = np.round(rng.uniform(0, 1, avail) * 64) / 64
        segs.append(s)
    run(segs, k, path=PATH_B)


def test_path_b_segment_longer_than_max_segment():
    """B': a segment longer than the declared bound takes the global-memory passes in the same launch"""
    rng = np.random.default_rng(11)
    segs = [rng.uniform(0, 1, 4000).astype(np.float32), bf16_logits(rng, 20000), np.full(9000, 0.5, np.float32)]
    for k in (1, 1025, 4096):
        run(segs, k, max_segment=4000, path=PATH_B)


# ------------------------------------------------------------------------------------------------------------------ path C
def test_path_c_unknown_and_in_between_bounds():
    """max_segment 0 (unknown) and 31 000 (above the LDS bound, at or below the multi-workgroup threshold)"""
    rng = np.random.default_rng(12)
    segs = [bf16_logits(rng, 32768), np.zeros(0, np.float32), np.float32([1.0]), np.full(5000, 0.5, np.float32),
            rng.uniform(0, 1, 31000).astype(np.float32)]
    for k in KS:
        run(segs, k, max_segment=0, path=PATH_C)
    run(segs, 1000, max_segment=31000, path=PATH_C)
    run(segs, 4096, min_score=0.0, max_segment=32768, path=PATH_C)


def test_path_c_more_segments_than_the_grid_holds():
    """65 536 small segments declared with max_segment > 32768: path A's grid cannot hold them, so one workgroup per segment"""
    from minddet_amd import det_ops

    rng = np.random.default_rng(13)
    L, n, k = 65536, 6, 4
    s = np.round(rng.uniform(-1, 1, (L, n)) * 4).astype(np.float32) / 4            # ties everywhere
    s[::7] = -0.0
    s[1::7, ::2] = 0.0
    off = np.arange(0, (L + 1) * n, n, dtype=np.int32)
    v, i, c = det_ops.topk_segmented(T(s.reshape(-1)), T(off), k, min_score=-0.5, max_segment=40000)
    assert last_path() == PATH_C
    v, i, c = v.cpu().numpy(), i.cpu().numpy(), c.cpu().numpy()
    sel = s > np.float32(-0.5)
    ri = np.argsort(-np.where(sel, s, -np.inf), axis=1, kind="stable")[:, :k]      # topk_desc_stable, row by row
    m = np.minimum(k, sel.sum(1))
    np.testing.assert_array_equal(c, m)
    live = np.arange(k)[None, :] < m[:, None]
    np.testing.assert_array_equal(np.where(live, i, -1), np.where(live, ri, -1))
    want_v = np.take_along_axis(s, ri, 1) + np.float32(0)                         # (-0.0 comes back as +0.0)
    np.testing.assert_array_equal(np.where(live, v, 7.0).astype(np.float32).view(np.uint32),
                                  np.where(live, want_v, 7.0).astype(np.float32).view(np.uint32))
    assert (v[~live] == -FLT_MAX).all() and (i[~live] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ values at the edges
@pytest.mark.parametrize("path,n", [(PATH_A, 40000), (PATH_B, 20000), (PATH_C, 20000)])
def test_signed_zeros_min_score_and_infinities(path, n):
    """+0.0 and -0.0 interleaved with equal neighbours (one value: ties go to the lower index whatever the sign), min_score 0.0 and
    -0.0 (neither zero is selectable), scores exactly equal to min_score (excluded), -inf (never selectable under the default
    min_score of -FLT_MAX, nor -FLT_MAX itself) and +inf (first)."""
    rng = np.random.default_rng(14 + path)
    ms_decl = {PATH_A: n, PATH_B: n, PATH_C: 0}[path]
    s = np.where(rng.uniform(0, 1, n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    s[rng.choice(n, 300, replace=False)] = rng.uniform(-1, 1, 300)
    s[5], s[6], s[7] = np.float32(-0.0), np.float32(0.0), np.float32(-0.0)
    t = s.copy()
    t[rng.choice(n, 200, replace=False)] = 0.25                       # == min_score below
    t[[10, 20, 30]] = [np.inf, -np.inf, np.inf]
    t[[40, 50]] = [-FLT_MAX, -np.inf]
    short = s[:3000].copy()                                               # (on path A: few candidates, the sort orders the zeros)
    for k in (1, 100, 1024, 4096):
        run([s, t, short], k, max_segment=ms_decl, path=path)             # zeros tie across signs (k > #positives)
        run([s, t, short], k, min_score=0.0, max_segment=ms_decl, path=path)
        run([s, t, short], k, min_score=-0.0, max_segment=ms_decl, path=path)
        run([t], k, min_score=0.25, max_segment=ms_decl, path=path)
        run([t], k, min_score=-np.inf, max_segment=ms_decl, path=path)
