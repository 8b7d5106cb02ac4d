"""GPU: md_conv_bwd_weight and md_conv1x1_bwd_data (include/minddet_hip_convbwd.h) against the float64 judges of
tests/convbwd_contract.py on the tensors read back.  Outputs are pre-filled with 0xFF bytes (a NaN pattern: an element the kernel does
not write fails every comparison, and a channel of dx the kernel must leave alone still holds it afterwards).

The weight gradient as built: the kernel of md_conv1x1_bwd_weight with (tap, channel) as one axis of kernel^2 cin virtual columns, 128 of
them per workgroup column, a lane group of eight columns inside one tap loading its own shifted pixel; slabs of S = max(256,
16 ceil(ceil(P / 256) / 16)) pixels, 16 pixels per step; the second launch maps dw's column order and masks the blocks.  The data
gradient: 256 pixels per workgroup, 16 per wave and step, 128 input channels per workgroup column, the reduction over cout in quads.
Each shape below names the edge it hits.

Conditions, fixed beforehand (the data kinds are those of tests/train_cases.py):
  small-int, sixteen-bit   bit for bit (the exact result is an fp32 number under any summation order; sixteen-bit: P <= 64 for the
                           weight gradient, cout <= 64 and w integers in [-4, 4] for the data gradient)
  gaussian                 weight gradient: train_contract.wgrad_bound, |dw - dw64| <= (2^-16 + L 2^-24) sum_p |dy x|;
                           data gradient: |dx - dx64| <= Ld 2^-24 sum_o |dy w|, Ld = cout
  kernel 1, korder 0, dense: the bytes of md_conv1x1_bwd_weight on the shapes of tests/test_conv_bwd_gpu.py
  padding, off-block elements and masked elements exactly +0.0; bit-identical results across three calls, a second stream and the pool
  / workspace forms."""
import numpy as np
import pytest
import torch

from tests import convbwd_contract as cc, train_cases, train_contract as tc
from tests.conftest import has_gpu
from tests.test_conv_bwd_gpu import SHAPES as K1_SHAPES, device_inputs, run as run_1x1
from tests.train_cases import shape

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"

# (shape, korder) of the 3x3 weight gradient
K3_SHAPES = {
    # P = 70: the boundary between the two images (pixel 35) lies inside the third 16-pixel step of the one slab: a tap of a border pixel
    # reads zero, not the other image's pixel next to it in memory
    "N 2, H 5, W 7, cin 8, cout 20": (shape(2, 5, 7, 8, 20), 0),
    # a single row / single pixels: the taps above and below (and, W = 1, beside) are +0.0 as a whole
    "N 1, H 1, W 9": (shape(1, 1, 9, 8, 3), 0),
    "N 3, H 1, W 1": (shape(3, 1, 1, 8, 3), 0),
    # P = 300: two slabs, the cut (pixel 256) inside row 12, so the neighbours of the pixels at the cut lie in the other slab; 576 virtual
    # columns = 4.5 workgroup columns, three row tiles of 64
    "H 15, W 20, cin 64, cout 192 (two slabs)": (shape(1, 15, 20, 64, 192), 1),
    # both column orders; cout 33: one row past two MFMA tiles; dy rows of 40 floats from channel 3 on
    "cin 128, cout 33 of 40 from 3, korder 0": (shape(2, 5, 7, 128, 33, Cy=40, dy_c_off=3), 0),
    "cin 128, cout 33 of 40 from 3, korder 1": (shape(2, 5, 7, 128, 33, Cy=40, dy_c_off=3), 1),
    # Cx = 44: pixel rows of x are not 16-byte aligned, the 2-byte load path
    "cin 40 of 44 from 4 (unaligned x rows)": (shape(2, 5, 7, 40, 20, Cx=44, x_c_off=4, Cy=24), 0),
    # P = 66048 > 256 x 256: the slab grows to 272 pixels, which is no multiple of W
    "N 1, H 258, W 256, cin 8, cout 1 (slabs of 272)": (shape(1, 258, 256, 8, 1), 0),
}
K3_SIXTEEN = {
    "P 60, two images, cin 8, cout 20": (shape(2, 5, 6, 8, 20), 0),
    "P 63, cin 64, cout 33 of 40 from 3, korder 1": (shape(1, 7, 9, 64, 33, Cy=40, dy_c_off=3), 1),
    "N 1, H 1, W 9": (shape(1, 1, 9, 16, 5), 0),
}
BLOCKS = [(0, 5, 0, 8), (5, 2, 8, 8), (7, 2, 16, 8)]                      # cout 9 as 5 + 2 + 2, cin 24 as 3 x 8
BLOCK_SHAPE = shape(2, 5, 7, 24, 9, Cy=16)


def filled(shp):
    return torch.full(shp, -1, dtype=torch.int32, device=DEV).view(torch.float32)


def pads(s, k):
    """rows and columns of the output: a pack's shape, wider than the layer in both directions"""
    return -(-s["cout"] // 32) * 32, -(-(k * k * s["cin"]) // 64) * 64 + 64


def run(s, x, dy, k, korder=0, blocks=(), with_db=True, workspace=True, stream=None):
    """-> (dw [rows,kpad], db [rows] or None) f32 numpy, outputs pre-filled with 0xFF"""
    from minddet_amd import det_ops, nn_ops

    rows, kpad = pads(s, k)
    pc = nn_ops.PackedConv(torch.empty((rows, kpad), dtype=torch.bfloat16, device=DEV), torch.empty((rows,), dtype=torch.float32, device=DEV),
                           s["cin"], s["cout"], k, k, 1, (k - 1) // 2, 0)
    pc.korder = korder
    dw, db = filled((rows, kpad)), filled((rows,)) if with_db else None
    call = lambda: det_ops.conv_bwd_weight(x, dy, pc, x_c_off=s["x_c_off"], dy_c_off=s["dy_c_off"], blocks=blocks, out=(dw, db), workspace=workspace)
    if stream is None:
        call()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            call()
        torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    return dw.cpu().numpy(), None if db is None else db.cpu().numpy()


def judge(s, x, dy, k, korder=0, blocks=()):
    rows, kpad = pads(s, k)
    return cc.wgrad_kxk(x, dy, s["cin"], s["cout"], kernel=k, korder=korder, x_c_off=s["x_c_off"], dy_c_off=s["dy_c_off"], blocks=blocks, rows=rows,
                        kpad=kpad)


def check_zeros(want, dw, db, cout):
    """padding, off-block elements and taps that never meet the image: +0.0, bit for bit"""
    assert (dw[~want["live"]].view(np.uint32) == 0).all() and (db[cout:].view(np.uint32) == 0).all()
    assert (dw[want["absdw"] == 0].view(np.uint32) == 0).all()


@pytest.mark.parametrize("name", list(K3_SHAPES))
def test_3x3_small_integers_are_exact(name):
    s, korder = K3_SHAPES[name]
    xd, dyd, x, dy = device_inputs("small-int", s)
    dw, db = run(s, xd, dyd, 3, korder)
    want = judge(s, x, dy, 3, korder)
    assert np.abs(want["dw"]).max() < 2 ** 24
    assert np.array_equal(dw.astype(np.float64), want["dw"]) and np.array_equal(db.astype(np.float64), want["db"])
    check_zeros(want, dw, db, s["cout"])
    if s["H"] == 1:                                                             # the six taps of the rows above and below
        col = cc.columns(3, s["cin"], korder)
        dead = np.concatenate([col[t] for t in (0, 1, 2, 6, 7, 8)] + ([col[3], col[5]] if s["W"] == 1 else []))
        assert not want["absdw"][:, dead].any() and np.count_nonzero(want["absdw"][:s["cout"], col[4]]) >= s["cout"] * s["cin"] // 2


@pytest.mark.parametrize("name", list(K3_SIXTEEN))
def test_3x3_sixteen_bit_dy_is_exact(name):
    """the data kind a dy rounded once to bf16 fails (tests/test_train_ops_cpu.py shows it on the CPU for the pointwise shapes)"""
    s, korder = K3_SIXTEEN[name]
    xd, dyd, x, dy = device_inputs("sixteen-bit", s)
    dw, db = run(s, xd, dyd, 3, korder)
    want = judge(s, x, dy, 3, korder)
    units = want["dw"] * 2.0 ** 20
    assert np.array_equal(units, np.round(units)) and (want["absdw"] * 2.0 ** 20).max() < 2 ** 24          # the exact result is an fp32 number
    differ = int((dw.astype(np.float64) != want["dw"]).sum())
    print(f"3x3 sixteen-bit[{name}]: {differ} of {int(want['live'].sum())} elements differ from the exact result")
    assert differ == 0 and np.array_equal(db.astype(np.float64), want["db"])
    check_zeros(want, dw, db, s["cout"])


@pytest.mark.parametrize("name", list(K3_SHAPES))
def test_3x3_gaussian_data_is_inside_the_bound(name):
    s, korder = K3_SHAPES[name]
    P = s["N"] * s["H"] * s["W"]
    xd, dyd, x, dy = device_inputs("gaussian", s)
    dw, db = run(s, xd, dyd, 3, korder)
    want = judge(s, x, dy, 3, korder)
    bw, bb = tc.wgrad_bound(P, want["absdw"]), tc.wgrad_bound(P, want["absdb"])
    ew, eb = np.abs(dw.astype(np.float64) - want["dw"]), np.abs(db.astype(np.float64) - want["db"])
    live = want["absdw"] > 0
    print(f"3x3 gaussian[{name}]: L = {tc.chain_length(P)}, worst error / bound dw {float((ew[live] / bw[live]).max()):.3e}, "
          f"db {float((eb[:s['cout']] / bb[:s['cout']]).max()):.3e}")
    assert np.isfinite(dw).all() and np.isfinite(db).all()
    assert (ew <= bw).all() and (eb <= bb).all()
    check_zeros(want, dw, db, s["cout"])


@pytest.mark.parametrize("name", list(K1_SHAPES))
def test_kernel_1_gives_the_bytes_of_the_pointwise_operator(name):
    s = K1_SHAPES[name]
    xd, dyd, _, _ = device_inputs("gaussian", s)
    rows, kpad = pads(s, 1)
    old = run_1x1(s, xd, dyd, rows, kpad)
    new = run(s, xd, dyd, 1)
    assert old[0].tobytes() == new[0].tobytes() and old[1].tobytes() == new[1].tobytes()
    assert np.isfinite(new[0]).all()


@pytest.mark.parametrize("kind", ["small-int", "gaussian"])
def test_block_diagonal_layer_stays_block_diagonal(kind):
    s = BLOCK_SHAPE
    P = s["N"] * s["H"] * s["W"]
    xd, dyd, x, dy = device_inputs(kind, s)
    dw, db = run(s, xd, dyd, 1, blocks=BLOCKS)
    want = judge(s, x, dy, 1, blocks=BLOCKS)
    assert want["live"].sum() == (5 + 2 + 2) * 8
    if kind == "small-int":
        assert np.array_equal(dw.astype(np.float64), want["dw"]) and np.array_equal(db.astype(np.float64), want["db"])
    else:
        assert (np.abs(dw.astype(np.float64) - want["dw"]) <= tc.wgrad_bound(P, want["absdw"])).all()
        assert (np.abs(db.astype(np.float64) - want["db"]) <= tc.wgrad_bound(P, want["absdb"])).all()
        dense = run(s, xd, dyd, 1)
        assert np.array_equal(dw[want["live"]], dense[0][want["live"]]) and dense[1].tobytes() == db.tobytes()     # the mask changes no live bit; db dense
        assert np.count_nonzero(dense[0]) > want["live"].sum()
    check_zeros(want, dw, db, s["cout"])
    assert np.count_nonzero(db[:s["cout"]]) == s["cout"]
    # the same mask on a 3x3 layer: every tap of an off-block pair is +0.0
    dw3, db3 = run(s, xd, dyd, 3, blocks=BLOCKS)
    want3 = judge(s, x, dy, 3, blocks=BLOCKS)
    assert want3["live"].sum() == 9 * 9 * 8
    check_zeros(want3, dw3, db3, s["cout"])
    assert (np.abs(dw3.astype(np.float64) - want3["dw"]) <= tc.wgrad_bound(P, want3["absdw"])).all()


@pytest.mark.parametrize("name", ["H 15, W 20, cin 64, cout 192 (two slabs)", "cin 128, cout 33 of 40 from 3, korder 0"])
def test_3x3_results_are_bit_identical_across_calls_streams_and_scratch_forms(name):
    s, korder = K3_SHAPES[name]
    xd, dyd, _, _ = device_inputs("gaussian", s)
    first = run(s, xd, dyd, 3, korder)
    side = torch.cuda.Stream(device=DEV)
    for kw in (dict(), dict(), dict(stream=side), dict(workspace=False), dict(workspace=False, stream=side)):
        again = run(s, xd, dyd, 3, korder, **kw)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes(), kw
    no_db = run(s, xd, dyd, 3, korder, with_db=False)
    assert no_db[1] is None and no_db[0].tobytes() == first[0].tobytes()


# ---------------------------------------------------------------------------------------------------- md_conv1x1_bwd_data
def dshape(N, H, W, cin, cout, Cy=None, dy_c_off=0, Cdx=None, dx_c_off=0, Ca=None, act_c_off=0):
    return dict(N=N, H=H, W=W, cin=cin, cout=cout, Cy=cout + dy_c_off if Cy is None else Cy, dy_c_off=dy_c_off,
                Cdx=cin + dx_c_off if Cdx is None else Cdx, dx_c_off=dx_c_off, Ca=cin + act_c_off if Ca is None else Ca, act_c_off=act_c_off)


D_SHAPES = {
    # P = 70: one workgroup row, the second step ragged (6 pixels in wave 0); cin 192: two workgroup columns, the second half empty;
    # cout 9: three o-quads, the last with one live row; dx at channels 8 .. 199 of 200 (aligned), dy rows of 16 from channel 3 on
    "P 70, cin 192, cout 9 of 16 from 3": dshape(2, 5, 7, 192, 9, Cy=16, dy_c_off=3, Cdx=200, dx_c_off=8),
    # one lane group, one product per element; dx rows of 13 floats from channel 3 and act rows of 12 from channel 4: the scalar paths
    "P 70, cin 8, cout 1 (unaligned dx and act)": dshape(2, 5, 7, 8, 1, Cdx=13, dx_c_off=3, Ca=12, act_c_off=4),
    # the limits: eight workgroup columns, 64 o-quads (the 64 KiB weight tile), two workgroup rows (the second 44 pixels)
    "P 300, cin 1024, cout 256": dshape(1, 15, 20, 1024, 256),
    "P 1": dshape(1, 1, 1, 24, 5, Cdx=32, dx_c_off=4),
}


def d_inputs(kind, s, with_act, seed=0):
    """-> device (dy f32, w bf16 [rows,kpad], act bf16 or None) and the same as fp32 numpy read back"""
    rng = np.random.default_rng([seed, s["N"], s["H"], s["W"], s["cin"], s["cout"]])
    pix = (s["N"], s["H"], s["W"])
    rows, kpad = -(-s["cout"] // 32) * 32, -(-s["cin"] // 64) * 64
    if kind == "small-int":
        dy, w = rng.integers(-8, 9, pix + (s["Cy"],)), rng.integers(-8, 9, (rows, kpad))
    elif kind == "sixteen-bit":
        assert s["cout"] <= 64
        odd, sign = 2 * rng.integers(0, 2 ** 15, pix + (s["Cy"],)) + 1, rng.integers(0, 2, pix + (s["Cy"],)) * 2 - 1
        dy, w = sign * odd * 2.0 ** -20, rng.integers(-4, 5, (rows, kpad))
    else:
        dy, w = rng.normal(0, 1, pix + (s["Cy"],)), tc.bf16_round(rng.normal(0, 1, (rows, kpad)).astype(np.float32))
    dyd = torch.from_numpy(np.asarray(dy, np.float32)).to(DEV)
    wd = torch.from_numpy(np.asarray(w, np.float32)).to(torch.bfloat16).to(DEV)
    actd = None
    if with_act:                                     # a ReLU's output: about half the elements +0, the rest positive bf16 numbers
        a = np.maximum(rng.normal(0, 1, pix + (s["Ca"],)), 0.0).astype(np.float32)
        actd = torch.from_numpy(a).to(torch.bfloat16).to(DEV)
    back = (dyd.cpu().numpy(), wd.float().cpu().numpy(), None if actd is None else actd.float().cpu().numpy())
    assert np.array_equal(back[0], np.asarray(dy, np.float32)) and np.array_equal(back[1], np.asarray(w, np.float32))
    return dyd, wd, actd, back


def d_run(s, dyd, wd, actd, stream=None):
    """-> dx [N,H,W,Cdx] f32 numpy, pre-filled with 0xFF"""
    from minddet_amd import det_ops, nn_ops

    pc = nn_ops.PackedConv(wd, None, s["cin"], s["cout"], 1, 1, 1, 0, 0)
    dx = filled((s["N"], s["H"], s["W"], s["Cdx"]))
    call = lambda: det_ops.conv1x1_bwd_data(dyd, pc, act=actd, dy_c_off=s["dy_c_off"], dx_c_off=s["dx_c_off"], act_c_off=s["act_c_off"] if actd is not None else 0,
                                            out=dx)
    if stream is None:
        call()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            call()
        torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    return dx.cpu().numpy()


def d_judge(s, back):
    dy, w, act = back
    return cc.dgrad_1x1(dy, w, s["cin"], s["cout"], act=act, dy_c_off=s["dy_c_off"], act_c_off=s["act_c_off"] if act is not None else 0)


def d_split(s, dx):
    """-> (the layer's channels, True where every other channel still holds the 0xFF fill)"""
    lo, hi = s["dx_c_off"], s["dx_c_off"] + s["cin"]
    rest = np.concatenate([dx[..., :lo], dx[..., hi:]], -1)
    return dx[..., lo:hi], bool((rest.view(np.uint32) == 0xFFFFFFFF).all())


D_EXACT = [(n, k, a) for n in D_SHAPES for k in ("small-int", "sixteen-bit") for a in (False, True) if k == "small-int" or D_SHAPES[n]["cout"] <= 64]


@pytest.mark.parametrize("name,kind,with_act", D_EXACT, ids=[f"{n}, {k}, {'act' if a else 'no act'}" for n, k, a in D_EXACT])
def test_dgrad_exact_data_is_bit_for_bit(name, kind, with_act):
    s = D_SHAPES[name]
    dyd, wd, actd, back = d_inputs(kind, s, with_act)
    got, untouched = d_split(s, d_run(s, dyd, wd, actd))
    want = d_judge(s, back)
    unit = 1.0 if kind == "small-int" else 2.0 ** 20
    assert np.array_equal(want["dx"] * unit, np.round(want["dx"] * unit)) and (want["absdx"] * unit).max() < 2 ** 24
    assert np.array_equal(got.astype(np.float64), want["dx"]) and untouched
    if with_act:
        assert 0.2 < want["keep"].mean() < 0.8 and (got[~want["keep"]].view(np.uint32) == 0).all()         # masked: +0.0, bit for bit


@pytest.mark.parametrize("name", list(D_SHAPES))
@pytest.mark.parametrize("with_act", [False, True], ids=["no act", "act"])
def test_dgrad_gaussian_data_is_inside_the_bound(name, with_act):
    s = D_SHAPES[name]
    dyd, wd, actd, back = d_inputs("gaussian", s, with_act)
    got, untouched = d_split(s, d_run(s, dyd, wd, actd))
    want = d_judge(s, back)
    err, bound = np.abs(got.astype(np.float64) - want["dx"]), cc.dgrad_bound(s["cout"], want["absdx"])
    live = want["absdx"] > 0
    print(f"dgrad gaussian[{name}, act {with_act}]: Ld = {cc.dgrad_chain_length(s['cout'])}, worst error / bound {float((err[live] / bound[live]).max()):.3e}")
    assert np.isfinite(got).all() and (err <= bound).all() and untouched
    if with_act:
        assert (got[~want["keep"]].view(np.uint32) == 0).all()


def test_dgrad_mask_edge_values():
    """+0, -0, a negative number, a NaN and the smallest positive bf16 in act: only the last lets the gradient through"""
    s = dshape(1, 2, 3, 8, 4)
    dyd, wd, _, back = d_inputs("small-int", s, False)
    bits = np.array([0x0000, 0x8000, 0xBF80, 0x7FC0, 0x0001, 0x3F80, 0xFF80, 0x7F80], np.uint16)          # +0 -0 -1 NaN min 1 -inf +inf
    act_bits = np.stack([np.roll(bits, p) for p in range(6)]).reshape(1, 2, 3, 8)
    actd = torch.from_numpy(act_bits.view(np.int16)).to(DEV).view(torch.bfloat16)
    act = (act_bits.astype(np.uint32) << 16).view(np.float32)
    got, untouched = d_split(s, d_run(s, dyd, wd, actd))
    want = cc.dgrad_1x1(back[0], back[1], 8, 4, act=act)
    assert want["keep"].sum() == 6 * 3 and np.array_equal(want["keep"], np.isin(act_bits, [0x0001, 0x3F80, 0x7F80]))
    assert np.array_equal(got.astype(np.float64), want["dx"]) and (got[~want["keep"]].view(np.uint32) == 0).all() and untouched
    plain = d_split(s, d_run(s, dyd, wd, None))[0]
    assert np.array_equal(plain[want["keep"]], got[want["keep"]]) and np.count_nonzero(plain[~want["keep"]]) > 0


def test_dgrad_results_are_bit_identical_across_calls_and_streams():
    s = D_SHAPES["P 70, cin 192, cout 9 of 16 from 3"]
    dyd, wd, actd, _ = d_inputs("gaussian", s, True)
    first = d_run(s, dyd, wd, actd)
    side = torch.cuda.Stream(device=DEV)
    for kw in (dict(), dict(), dict(stream=side)):
        assert d_run(s, dyd, wd, actd, **kw).tobytes() == first.tobytes(), kw
