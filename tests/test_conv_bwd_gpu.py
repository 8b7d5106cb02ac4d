"""GPU: md_conv1x1_bwd_weight (include/minddet_hip_train.h) against the float64 contract tests/train_contract.wgrad on the tensors read
back.  Outputs are pre-filled with 0xFF bytes (a NaN pattern: an element the kernel does not write fails every comparison).

The kernel as built: slabs of S = max(256, 16 ceil(ceil(P / 256) / 16)) pixels, four waves per workgroup walking 16 pixels per step and
loading four steps (64 pixels) ahead, 128 input channels per workgroup column, 16 / 32 / 64 output channels per workgroup row (cout <= 16,
<= 32, above), a second launch summing the slabs in 8 interleaved chains.  Each shape below names the edge it hits.

Conditions, fixed beforehand:
  small-int, sixteen-bit   bit for bit (the exact result is an fp32 number under any summation order; tests/test_train_ops_cpu.py shows on
                           the CPU that a dy rounded to bf16 misses the sixteen-bit result in over 90 % of the elements)
  gaussian                 |dw - dw64| <= (2^-16 + L 2^-24) sum_p |dy x|, L = train_contract.chain_length(P), the header's formula; db the
                           same with x = 1
  padding rows and columns exactly +0.0; bit-identical results across three calls, a second stream and the pool / workspace forms."""
import numpy as np
import pytest
import torch

from tests import train_cases, train_contract as tc
from tests.conftest import has_gpu
from tests.train_cases import shape

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"

SHAPES = {
    # P = 70: one slab, four full steps and a ragged fifth (6 pixels: waves 2, 3 idle, wave 1 half), the ring of four refilled once with
    # nothing; cin 40: five of a column's sixteen lane groups live; cout 20: two row tiles, 12 rows of the second dead; x from channel 8
    "P 70, cin 40 of 48 from 8, cout 20 of 24": shape(2, 5, 7, 40, 20, Cx=48, x_c_off=8, Cy=24),
    # P = 2145: nine slabs of 256 (more than the 8 chains of the sum: chain 0 adds two), the last one ragged (97 pixels); the production channels
    "P 2145, cin 384, cout 20": shape(1, 33, 65, 384, 20, Cy=24),
    # the limits, two slabs (the second 44 pixels): one lane group and one row live / eight workgroup columns and four rows of 64
    "P 300, cin 8, cout 1": shape(1, 15, 20, 8, 1),
    "P 300, cin 1024, cout 256": shape(1, 15, 20, 1024, 256),
    # cout 33: one row past two MFMA tiles (the 64-row form, R = 48: rows 48 .. 63 are computed and not stored); dy rows of 40 floats
    # from channel 3 on: no dy address is 16-byte aligned
    "P 70, cin 16, cout 33 of 40 from 3": shape(2, 5, 7, 16, 33, Cy=40, dy_c_off=3),
    "P 1": shape(1, 1, 1, 24, 5),
    # Cx = 44: pixel rows of x are not 16-byte aligned, the 2-byte load path
    "P 70, cin 40 of 44 from 4 (unaligned x rows)": shape(2, 5, 7, 40, 20, Cx=44, x_c_off=4, Cy=24),
    # P = 66048 > 256 x 256: the slab grows to 272 pixels (243 slabs, 31 additions per chain of the sum)
    "P 66048, cin 8, cout 1 (slabs of 272)": shape(1, 258, 256, 8, 1),
}


def run(s, x, dy, rows, kpad, with_db=True, workspace=True, stream=None):
    """-> (dw [rows,kpad], db [rows] or None) f32 numpy, outputs pre-filled with 0xFF"""
    from minddet_amd import det_ops, nn_ops

    pc = nn_ops.PackedConv(torch.empty((rows, kpad), dtype=torch.bfloat16, device=DEV), torch.empty((rows,), dtype=torch.float32, device=DEV),
                           s["cin"], s["cout"], 1, 1, 1, 0, 0)
    dw = torch.full((rows, kpad), -1, dtype=torch.int32, device=DEV).view(torch.float32)
    db = torch.full((rows,), -1, dtype=torch.int32, device=DEV).view(torch.float32) if with_db else None
    call = lambda: det_ops.conv1x1_bwd_weight(x, dy, pc, x_c_off=s["x_c_off"], dy_c_off=s["dy_c_off"], out=(dw, db), workspace=workspace)
    if stream is None:
        call()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            call()
        torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    return dw.cpu().numpy(), None if db is None else db.cpu().numpy()


def device_inputs(kind, s):
    x, dy = train_cases.data(kind, s)
    xd = torch.from_numpy(x).to(torch.bfloat16).to(DEV)
    dyd = torch.from_numpy(dy).to(DEV)
    back_x, back_dy = xd.float().cpu().numpy(), dyd.cpu().numpy()
    assert np.array_equal(back_x, x) and np.array_equal(back_dy, dy)          # the inputs are bf16 / fp32 numbers as they stand
    return xd, dyd, back_x, back_dy


def pads(s):
    """rows and columns of the output: a pack's shape, wider than the layer in both directions"""
    return -(-s["cout"] // 32) * 32, -(-s["cin"] // 64) * 64


def check_padding(s, dw, db):
    live = np.zeros(dw.shape, bool)
    live[:s["cout"], :s["cin"]] = True
    assert (dw[~live].view(np.uint32) == 0).all() and (db[s["cout"]:].view(np.uint32) == 0).all()      # +0.0, bit for bit


@pytest.mark.parametrize("name", list(SHAPES))
def test_small_integers_are_exact(name):
    s = SHAPES[name]
    xd, dyd, x, dy = device_inputs("small-int", s)
    rows, kpad = pads(s)
    dw, db = run(s, xd, dyd, rows, kpad)
    want = tc.wgrad(x, dy, s["cin"], s["cout"], s["x_c_off"], s["dy_c_off"], rows, kpad)
    assert np.abs(want["dw"]).max() < 2 ** 24
    assert np.array_equal(dw.astype(np.float64), want["dw"]) and np.array_equal(db.astype(np.float64), want["db"])
    check_padding(s, dw, db)


@pytest.mark.parametrize("name", list(train_cases.SIXTEEN_BIT_SHAPES))
def test_sixteen_bit_dy_is_exact(name):
    """the case a dy rounded once to bf16 fails"""
    s = train_cases.SIXTEEN_BIT_SHAPES[name]
    xd, dyd, x, dy = device_inputs("sixteen-bit", s)
    rows, kpad = pads(s)
    dw, db = run(s, xd, dyd, rows, kpad)
    want = tc.wgrad(x, dy, s["cin"], s["cout"], s["x_c_off"], s["dy_c_off"], rows, kpad)
    differ = int((dw.astype(np.float64) != want["dw"]).sum())
    print(f"sixteen-bit[{name}]: {differ} of {s['cin'] * s['cout']} elements differ from the exact result")
    assert differ == 0 and np.array_equal(db.astype(np.float64), want["db"])
    check_padding(s, dw, db)


@pytest.mark.parametrize("name", list(SHAPES))
def test_gaussian_data_is_inside_the_bound(name):
    s = SHAPES[name]
    P = s["N"] * s["H"] * s["W"]
    xd, dyd, x, dy = device_inputs("gaussian", s)
    rows, kpad = pads(s)
    dw, db = run(s, xd, dyd, rows, kpad)
    want = tc.wgrad(x, dy, s["cin"], s["cout"], s["x_c_off"], s["dy_c_off"], rows, kpad)
    bw, bb = tc.wgrad_bound(P, want["absdw"]), tc.wgrad_bound(P, want["absdb"])
    ew, eb = np.abs(dw.astype(np.float64) - want["dw"]), np.abs(db.astype(np.float64) - want["db"])
    live = want["absdw"] > 0
    print(f"gaussian[{name}]: L = {tc.chain_length(P)}, worst error / bound dw {float((ew[live] / bw[live]).max()):.3e}, "
          f"db {float((eb[:s['cout']] / bb[:s['cout']]).max()):.3e}")
    assert np.isfinite(dw).all() and np.isfinite(db).all()
    assert (ew <= bw).all() and (eb <= bb).all()
    check_padding(s, dw, db)


@pytest.mark.parametrize("name", ["P 2145, cin 384, cout 20", "P 70, cin 16, cout 33 of 40 from 3"])
def test_results_are_bit_identical_across_calls_streams_and_scratch_forms(name):
    s = SHAPES[name]
    xd, dyd, _, _ = device_inputs("gaussian", s)
    rows, kpad = pads(s)
    first = run(s, xd, dyd, rows, kpad)
    side = torch.cuda.Stream(device=DEV)
    for kw in (dict(), dict(), dict(stream=side), dict(workspace=False), dict(workspace=False, stream=side)):
        again = run(s, xd, dyd, rows, kpad, **kw)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes(), kw
    no_db = run(s, xd, dyd, rows, kpad, with_db=False)
    assert no_db[1] is None and no_db[0].tobytes() == first[0].tobytes()
