"""The seeded inputs that tests/test_train_ops_cpu.py and tests/test_conv_bwd_gpu.py share for md_conv1x1_bwd_weight: three kinds of data
on one shape description.  A shape is dict(N, H, W, cin, cout, Cx, x_c_off, Cy, dy_c_off).

  small-int    x and dy integers in [-8, 8]: every product and every partial sum is a small integer, so any summation order and any
               operand precision of 8 bits or more gives the same bits
  sixteen-bit  dy = +-(odd integers below 2^16) 2^-20, x integers in [-4, 4], P <= 64: each product needs 16 + 3 bits, each partial sum
               stays below 64 x 65535 x 4 < 2^24 units of 2^-20, so fp32 accumulation is exact in any order -- and a dy rounded to
               bf16 (8 bits) loses the low bits of every value: the data a bf16-rounded operand fails
  gaussian     dy N(0, 1) with full fp32 mantissas, x the fp32 values of bf16 N(0, 1)
Channels outside the layer's ranges carry values of the same kind (they must not enter the result)."""
import numpy as np

from tests import train_contract as tc


def shape(N, H, W, cin, cout, Cx=None, x_c_off=0, Cy=None, dy_c_off=0):
    return dict(N=N, H=H, W=W, cin=cin, cout=cout, Cx=cin + x_c_off if Cx is None else Cx, x_c_off=x_c_off,
                Cy=cout + dy_c_off if Cy is None else Cy, dy_c_off=dy_c_off)


SIXTEEN_BIT_SHAPES = {
    "P 64, cin 40, cout 20": shape(1, 8, 8, 40, 20, Cx=48, x_c_off=8, Cy=24),
    "P 35, cin 8, cout 33, unaligned dy rows": shape(1, 5, 7, 8, 33, Cy=40, dy_c_off=3),
}


def data(kind, s, seed=0):
    """-> (x [N,H,W,Cx] f32 holding bf16 values, dy [N,H,W,Cy] f32)"""
    rng = np.random.default_rng([seed, s["N"], s["H"], s["W"], s["cin"], s["cout"]])
    xs, ds = (s["N"], s["H"], s["W"], s["Cx"]), (s["N"], s["H"], s["W"], s["Cy"])
    if kind == "small-int":
        return rng.integers(-8, 9, xs).astype(np.float32), rng.integers(-8, 9, ds).astype(np.float32)
    if kind == "sixteen-bit":
        assert s["N"] * s["H"] * s["W"] <= 64
        odd = 2 * rng.integers(0, 2 ** 15, ds) + 1
        sign = rng.integers(0, 2, ds) * 2 - 1
        return rng.integers(-4, 5, xs).astype(np.float32), (sign * odd * 2.0 ** -20).astype(np.float32)
    if kind == "gaussian":
        return tc.bf16_round(rng.normal(0, 1, xs).astype(np.float32)), rng.normal(0, 1, ds).astype(np.float32)
    raise ValueError(kind)
