"""GPU: md_conv2d_grouped_bwd_data and md_conv2d_grouped_bwd_weight (include/minddet_hip_groupedbwd.h) against the float64 judges of
tests/groupedbwd_contract.py on the tensors read back.  Outputs are pre-filled with 0xFF bytes (a NaN pattern: an element the kernel does
not write fails every comparison, and a channel of dx the kernel must leave alone still holds it afterwards).

The data gradient as built: a workgroup owns MD_GROUPED_BWD_TILE = 64 consecutive pixels of the flat index (n, h, w) (a 1 x 64 tile
that wraps over rows and images) and walks four groups; a wave takes 16 of the pixels; every lane tests its own tap against its own
image.  The weight gradient: md_conv_bwd_weight's kernel with the group as a grid dimension, slabs of S = max(256, ..)
pixels.  Each shape below names the edge it hits.

Conditions, fixed beforehand:
  small-int (|dy|, |w|, |x| <= 4)   bit for bit (the exact result is an fp32 number under any summation order)
  gaussian                          data gradient: |dx - dx64| <= Ld 2^-24 sum |dy w|, Ld = k k cout, on EVERY element;
                                    weight gradient: |dw - dw64| <= L(P) 2^-24 sum_p |dy x| on every element (db: x = 1)
  group g's rows of dw and db       the bytes of one md_conv_bwd_weight call for that group
  masked elements, rows no group owns: +0.0, bit for bit; channels no group covers: the 0xFF fill; bit-identical results across three
  calls, a second stream, the pool / workspace forms and an unaligned act / dx base."""
import numpy as np
import pytest
import torch

from tests import groupedbwd_contract as gc, train_contract as tc
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
TILE = 64

# three groups of cout 1 / 2 / 3, y_off unordered and gapped in 12 channels of dy, rows of w unordered with rows 6 and 7 owned by no
# group, the groups' slices at channels 8 .. 199 of 208
BASE = dict(couts=(1, 2, 3), y_offs=(9, 0, 4), w_rows=(5, 0, 2), R=8, Cy=12, x_c_off=8, C=208)
NUSC_COUTS = [c for nc in (1, 2, 2, 1, 2, 2) for c in (2, 1, 3, 2, 2, nc)]          # reg, height, dim, rot, vel, hm per task: 70 channels


def case(N, H, W, k=3, **kw):
    s = dict(BASE, N=N, H=H, W=W, k=k)
    s.update(kw)
    return s


def nusc(N, H, W):
    offs = [sum(NUSC_COUTS[:g]) for g in range(36)]
    return dict(N=N, H=H, W=W, k=3, couts=NUSC_COUTS, y_offs=offs, w_rows=offs, R=70, Cy=72, x_c_off=0, C=2304)


SHAPES = {
    # P = 70: image borders and the seam between the two images (pixel 35) lie inside one 16-pixel step
    "N 2, H 5, W 7": case(2, 5, 7),
    # a single pixel (only the centre tap meets the image), a single row of 17 (one pixel past a step), one pixel past the tile in both
    # directions (tile cuts inside both rows, the last workgroup holds two pixels)
    "N 3, H 1, W 1": case(3, 1, 1),
    "N 1, H 1, W 17": case(1, 1, 17),
    "N 1, H 2, W 65 (tile + 1)": case(1, 2, TILE + 1),
    "k 1": case(2, 5, 7, k=1),
    # the forward operator's limit: one group of 16 outputs (four o-quads) beside a narrow one
    "cout 16": case(2, 5, 7, couts=(16, 3), y_offs=(0, 17), w_rows=(3, 0), R=19, Cy=20, C=136),
    # the nuScenes table: 36 groups (nine walks of four), 70 of 72 channels of dy, 2304 channels
    "nuScenes table, 16 x 16": nusc(1, 16, 16),
    # P = 300: two slabs of the weight gradient, the cut (pixel 256) inside row 12
    "H 15, W 20 (two slabs)": case(1, 15, 20),
}


def table(s):
    return gc.table(s["k"], s["couts"], s["y_offs"], s["w_rows"], s["x_c_off"])


def filled(shp, dtype=torch.float32):
    return torch.full(shp, -1, dtype=torch.int32, device=DEV).view(dtype)


_INPUTS = {}


def inputs(kind, name):
    """-> device (dy f32, w bf16 [R, k k 64], act bf16 [N,H,W,C]: a ReLU's output) and the same as fp32 numpy read back; made once"""
    if (kind, name) not in _INPUTS:
        s = SHAPES[name]
        rng = np.random.default_rng([len(name), s["N"], s["H"], s["W"], s["k"], kind == "gaussian"])
        pix, kk = (s["N"], s["H"], s["W"]), s["k"] * s["k"] * 64
        if kind == "small-int":
            dy, w, a = rng.integers(-4, 5, pix + (s["Cy"],)), rng.integers(-4, 5, (s["R"], kk)), np.maximum(rng.integers(-4, 5, pix + (s["C"],)), 0)
        else:
            dy, w, a = rng.normal(0, 1, pix + (s["Cy"],)), rng.normal(0, 1, (s["R"], kk)), np.maximum(rng.normal(0, 1, pix + (s["C"],)), 0.0)
        dyd = torch.from_numpy(np.asarray(dy, np.float32)).to(DEV)
        wd = torch.from_numpy(np.asarray(w, np.float32)).to(torch.bfloat16).to(DEV)
        ad = torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).to(DEV)
        _INPUTS[(kind, name)] = (dyd, wd, ad, (dyd.cpu().numpy(), wd.float().cpu().numpy(), ad.float().cpu().numpy()))
    return _INPUTS[(kind, name)]


def pack(s, wd):
    from minddet_amd import nn_ops

    return nn_ops.PackedGrouped(wd, torch.zeros((s["R"],), dtype=torch.float32, device=DEV), s["k"], s["couts"], s["w_rows"], s["y_offs"], 0)


def on(stream, call):
    if stream is None:
        call()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            call()
        torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()


def d_run(s, dyd, wd, actd, stream=None, out=None):
    """-> dx [N,H,W,C] f32 numpy, pre-filled with 0xFF"""
    from minddet_amd import det_ops

    dx = filled((s["N"], s["H"], s["W"], s["C"])) if out is None else out
    on(stream, lambda: det_ops.conv2d_grouped_bwd_data(dyd, pack(s, wd), act=actd, x_c_off=s["x_c_off"], out=dx))
    return dx.cpu().numpy()


def d_check_rest(s, want, got):
    """(d): every channel no group covers still holds the 0xFF fill"""
    assert want["covered"].sum() == 64 * len(s["couts"]) and (got[..., ~want["covered"]].view(np.uint32) == 0xFFFFFFFF).all()


D_NAMES = [n for n in SHAPES if "two slabs" not in n]


@pytest.mark.parametrize("with_act", [False, True], ids=["no act", "act"])
@pytest.mark.parametrize("name", D_NAMES)
def test_dgrad_small_integers_are_bit_for_bit(name, with_act):
    s = SHAPES[name]
    dyd, wd, ad, (dy, w, a) = inputs("small-int", name)
    got = d_run(s, dyd, wd, ad if with_act else None)
    want = gc.dgrad_grouped(dy, w, table(s), act=a if with_act else None, cdx=s["C"])
    assert np.abs(want["absdx"]).max() < 2 ** 24 and np.count_nonzero(want["dx"]) > 0
    cov = want["covered"]
    assert np.array_equal(got[..., cov].astype(np.float64), want["dx"][..., cov])
    d_check_rest(s, want, got)
    if with_act:
        assert 0.2 < want["keep"][..., cov].mean() < 0.8 and (got[..., cov][~want["keep"][..., cov]].view(np.uint32) == 0).all()     # +0.0, bit for bit


@pytest.mark.parametrize("with_act", [False, True], ids=["no act", "act"])
@pytest.mark.parametrize("name", D_NAMES)
def test_dgrad_gaussian_data_is_inside_the_bound_on_every_element(name, with_act):
    s = SHAPES[name]
    dyd, wd, ad, (dy, w, a) = inputs("gaussian", name)
    got = d_run(s, dyd, wd, ad if with_act else None)
    want = gc.dgrad_grouped(dy, w, table(s), act=a if with_act else None, cdx=s["C"])
    cov = want["covered"]
    err, bound = np.abs(got[..., cov].astype(np.float64) - want["dx"][..., cov]), gc.dgrad_bound(want)[..., cov]
    live = bound > 0
    print(f"grouped dgrad gaussian[{name}, act {with_act}]: Ld up to {int(want['ld'].max())}, worst error / bound {float((err[live] / bound[live]).max()):.3e}")
    assert np.isfinite(got[..., cov]).all() and (err <= bound).all()
    d_check_rest(s, want, got)
    if with_act:
        assert (got[..., cov][~want["keep"][..., cov]].view(np.uint32) == 0).all()


def test_dgrad_mask_edge_values():
    """(c) +0, -0, a negative number, a NaN and the smallest positive bf16 planted in act: only act > 0 lets the gradient through"""
    name = "N 2, H 5, W 7"
    s = SHAPES[name]
    dyd, wd, _, (dy, w, _) = inputs("small-int", name)
    bits = np.array([0x0000, 0x8000, 0xBF80, 0x7FC0, 0x0001, 0x3F80, 0xFF80, 0x7F80], np.uint16)          # +0 -0 -1 NaN min 1 -inf +inf
    P = s["N"] * s["H"] * s["W"]
    act_bits = np.stack([np.roll(np.tile(bits, s["C"] // 8), p) for p in range(P)]).reshape(s["N"], s["H"], s["W"], s["C"])
    actd = torch.from_numpy(act_bits.view(np.int16)).to(DEV).view(torch.bfloat16)
    act = (act_bits.astype(np.uint32) << 16).view(np.float32)
    got = d_run(s, dyd, wd, actd)
    want = gc.dgrad_grouped(dy, w, table(s), act=act, cdx=s["C"])
    cov = want["covered"]
    assert np.array_equal(want["keep"][..., cov], np.isin(act_bits, [0x0001, 0x3F80, 0x7F80])[..., cov])
    assert np.array_equal(got[..., cov].astype(np.float64), want["dx"][..., cov]) and (got[..., cov][~want["keep"][..., cov]].view(np.uint32) == 0).all()
    plain = d_run(s, dyd, wd, None)
    keep = want["keep"]
    assert np.array_equal(plain[keep], got[keep]) and np.count_nonzero(plain[..., cov][~keep[..., cov]]) > 0
    d_check_rest(s, want, got)


@pytest.mark.parametrize("name", ["N 2, H 5, W 7", "k 1"])
def test_dgrad_unaligned_act_and_dx_take_the_element_path_bit_identically(name):
    """(i) act 2 bytes and dx 4 bytes off their 16-byte boundaries; w 2 bytes off its 8-byte boundary"""
    from minddet_amd import det_ops

    s = SHAPES[name]
    dyd, wd, ad, _ = inputs("gaussian", name)
    first = d_run(s, dyd, wd, ad)
    shp = (s["N"], s["H"], s["W"], s["C"])
    n = int(np.prod(shp))
    dx_flat, act_flat, w_flat = filled((n + 1,)), torch.empty((n + 1,), dtype=torch.bfloat16, device=DEV), torch.empty((wd.numel() + 1,), dtype=torch.bfloat16, device=DEV)
    dx, act, w = dx_flat[1:].view(shp), act_flat[1:].view(shp), w_flat[1:].view(wd.shape)
    act.copy_(ad)
    w.copy_(wd)
    assert dx.data_ptr() % 16 == 4 and act.data_ptr() % 16 == 2 and w.data_ptr() % 8 == 2 and dx.is_contiguous() and act.is_contiguous()
    det_ops.conv2d_grouped_bwd_data(dyd, pack(s, w), act=act, x_c_off=s["x_c_off"], out=dx)
    torch.cuda.synchronize()
    assert dx.cpu().numpy().tobytes() == first.tobytes()
    assert dx_flat[:1].view(torch.int32).item() == -1                                                       # the element in front of dx


def test_dgrad_results_are_bit_identical_across_calls_and_streams():
    name = "nuScenes table, 16 x 16"
    s = SHAPES[name]
    dyd, wd, ad, _ = inputs("gaussian", name)
    first = d_run(s, dyd, wd, ad)
    side = torch.cuda.Stream(device=DEV)
    for kw in (dict(), dict(), dict(stream=side)):
        assert d_run(s, dyd, wd, ad, **kw).tobytes() == first.tobytes(), kw


# ---------------------------------------------------------------------------------------------------- md_conv2d_grouped_bwd_weight
W_NAMES = ["N 2, H 5, W 7", "N 3, H 1, W 1", "N 1, H 1, W 17", "k 1", "cout 16", "nuScenes table, 16 x 16", "H 15, W 20 (two slabs)"]


def w_run(s, xd, dyd, with_db=True, workspace=True, stream=None):
    """-> (dw [R, k k 64], db [R] or None) f32 numpy, outputs pre-filled with 0xFF"""
    from minddet_amd import det_ops

    pk = pack(s, torch.empty((s["R"], s["k"] * s["k"] * 64), dtype=torch.bfloat16, device=DEV))
    dw, db = filled((s["R"], s["k"] * s["k"] * 64)), filled((s["R"],)) if with_db else None
    on(stream, lambda: det_ops.conv2d_grouped_bwd_weight(xd, dyd, pk, x_c_off=s["x_c_off"], out=(dw, db), with_bias=with_db, workspace=workspace))
    return dw.cpu().numpy(), None if db is None else db.cpu().numpy()


def w_check_zeros(want, dw, db):
    """rows no group owns and taps that never meet the image: +0.0, bit for bit"""
    assert (dw[~want["live"]].view(np.uint32) == 0).all() and (db[~want["live"]].view(np.uint32) == 0).all()
    assert (dw[want["absdw"] == 0].view(np.uint32) == 0).all()


@pytest.mark.parametrize("name", W_NAMES)
def test_wgrad_small_integers_are_exact(name):
    s = SHAPES[name]
    dyd, _, xd, (dy, _, x) = inputs("small-int", name)
    dw, db = w_run(s, xd, dyd)
    want = gc.wgrad_grouped(x, dy, table(s), s["R"])
    assert np.abs(want["absdw"]).max() < 2 ** 24 and want["live"].sum() == sum(s["couts"])
    assert np.array_equal(dw.astype(np.float64), want["dw"]) and np.array_equal(db.astype(np.float64), want["db"])
    w_check_zeros(want, dw, db)


@pytest.mark.parametrize("name", W_NAMES)
def test_wgrad_gaussian_data_is_inside_the_bound_and_each_group_is_the_single_call(name):
    from minddet_amd import det_ops, nn_ops

    s = SHAPES[name]
    P, k = s["N"] * s["H"] * s["W"], s["k"]
    dyd, _, xd, (dy, _, x) = inputs("gaussian", name)
    dw, db = w_run(s, xd, dyd)
    want = gc.wgrad_grouped(x, dy, table(s), s["R"])
    L = tc.chain_length(P)
    bw, bb = L * 2.0 ** -24 * want["absdw"], L * 2.0 ** -24 * want["absdb"]
    ew, eb = np.abs(dw.astype(np.float64) - want["dw"]), np.abs(db.astype(np.float64) - want["db"])
    print(f"grouped wgrad gaussian[{name}]: L = {L}, worst error / bound dw {float((ew[bw > 0] / bw[bw > 0]).max()):.3e}, "
          f"db {float((eb[bb > 0] / bb[bb > 0]).max()):.3e}")
    assert np.isfinite(dw).all() and np.isfinite(db).all() and (ew <= bw).all() and (eb <= bb).all()
    w_check_zeros(want, dw, db)
    # group g alone through md_conv_bwd_weight: kernel k, korder 0, cin 64, x_c_off + 64 g, dy_c_off = y_off[g], cout[g]
    pc = nn_ops.PackedConv(torch.empty((16, k * k * 64), dtype=torch.bfloat16, device=DEV), torch.empty((16,), dtype=torch.float32, device=DEV),
                           64, 16, k, k, 1, (k - 1) // 2, 0)
    pc.korder = 0
    groups = range(len(s["couts"])) if len(s["couts"]) <= 3 else (0, 17, 35)
    for g in groups:
        co, r0 = s["couts"][g], s["w_rows"][g]
        one_w, one_b = filled((16, k * k * 64)), filled((16,))
        det_ops.conv_bwd_weight(xd, dyd, pc, x_c_off=s["x_c_off"] + 64 * g, dy_c_off=s["y_offs"][g], cout=co, out=(one_w, one_b))
        torch.cuda.synchronize()
        assert one_w[:co].cpu().numpy().tobytes() == dw[r0:r0 + co].tobytes() and one_b[:co].cpu().numpy().tobytes() == db[r0:r0 + co].tobytes(), g


@pytest.mark.parametrize("name", ["H 15, W 20 (two slabs)", "nuScenes table, 16 x 16"])
def test_wgrad_results_are_bit_identical_across_calls_streams_and_scratch_forms(name):
    from minddet_amd import _lib, det_ops

    s = SHAPES[name]
    dyd, _, xd, _ = inputs("gaussian", name)
    first = w_run(s, xd, dyd)
    side = torch.cuda.Stream(device=DEV)
    for kw in (dict(), dict(), dict(stream=side), dict(workspace=False), dict(workspace=False, stream=side)):
        again = w_run(s, xd, dyd, **kw)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes(), kw
    no_db = w_run(s, xd, dyd, with_db=False)
    assert no_db[1] is None and no_db[0].tobytes() == first[0].tobytes()
    # exactly the bytes the library answers, cut out of a block of 0xA5: both sides stay untouched
    P, G, k = s["N"] * s["H"] * s["W"], len(s["couts"]), s["k"]
    n, guard = det_ops.conv2d_grouped_bwd_weight_workspace_bytes(P, G, k), 4096
    block = torch.full((guard + n + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    dw, db = filled((s["R"], k * k * 64)), filled((s["R"],))
    pk = pack(s, torch.empty((s["R"], k * k * 64), dtype=torch.bfloat16, device=DEV))
    _lib.call("md_conv2d_grouped_bwd_weight", [xd, dyd, dw, db, block[guard:guard + n]], extra=pk.attrs(s["x_c_off"]))
    torch.cuda.synchronize()
    assert bool((block[:guard] == 0xA5).all()) and bool((block[guard + n:] == 0xA5).all())
    assert dw.cpu().numpy().tobytes() == first[0].tobytes() and db.cpu().numpy().tobytes() == first[1].tobytes()
    with pytest.raises(_lib.MindDetHipError, match="rc=4"):
        _lib.call("md_conv2d_grouped_bwd_weight", [xd, dyd, dw, db, block[guard:guard + n - 1]], extra=pk.attrs(s["x_c_off"]))
