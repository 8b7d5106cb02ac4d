"""Shared by the tests that hold a conv launch to tests/conv_contract.py (test_conv_production_gpu.py, test_centerpoint_conv_gpu.py,
test_c3pair_gpu.py, test_pw_chain_gpu.py and, for the data draws, test_conv_reference_cpu.py): the two regimes' value draws, the
sentinel-filled output with guard zones, and the comparison of an output with a reference of conv_contract."""
import torch

SENTINEL = 0x7FA5          # a bf16 NaN bit pattern (as int16) that no computed value takes
GUARD = 1 << 16            # sentinel elements on each side of the output tensor


def sentinel_out(shape, device):
    """(y, flat): an output tensor of `shape` filled with the sentinel, inside a sentinel buffer GUARD elements longer on each side"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int16, device=device)
    return flat[GUARD:GUARD + n].view(torch.bfloat16).view(shape), flat


def check_guards(flat):
    assert bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[-GUARD:] == SENTINEL).all()), "write outside the output tensor"


class Data:
    """the two regimes' value draws (on `device`, from one generator per case)"""

    def __init__(self, exact, seed, device):
        self.exact, self.device = exact, device
        self.g = torch.Generator(device=device).manual_seed(seed)

    def act(self, shape, hi=2):
        if self.exact:
            return torch.randint(-hi, hi + 1, shape, generator=self.g, device=self.device, dtype=torch.int16).to(torch.bfloat16)
        return torch.randn(shape, generator=self.g, device=self.device).to(torch.bfloat16)

    def weight(self, shape, k, silu=False):
        """logical weight, bf16 values (exact: {-1, 0, 1} 2^-s; s > 0 only for SiLU layers, to keep the pre-activation near 0)"""
        if self.exact:
            s = max(0, round(0.5 * torch.log2(torch.tensor(4.0 * k / 3 / 16)).item())) if silu else 0
            w = torch.randint(-1, 2, shape, generator=self.g, device=self.device, dtype=torch.int16).float() * 2.0 ** -s
        else:
            w = torch.randn(shape, generator=self.g, device=self.device) / k ** 0.5
        return w.to(torch.bfloat16)

    def bias(self, n, n_pad):
        b = torch.zeros((n_pad,), dtype=torch.float32, device=self.device)
        if self.exact:
            b[:n] = torch.randint(-3, 4, (n,), generator=self.g, device=self.device).float()
        else:
            b[:n] = torch.randn((n,), generator=self.g, device=self.device)
        return b


def check(got, ref, exact):
    """got against a reference: exact -> float64 bf16 values, bit for bit; else (y, bound) -> worst err / bound"""
    if exact:
        want = ref.to(torch.bfloat16).view(torch.int16)
        bad = got.contiguous().view(torch.int16) != want
        nbad = int(bad.sum())
        assert not nbad, f"{nbad} of {bad.numel()} outputs differ; first at {tuple(int(v) for v in bad.nonzero()[0])}"
        return 0.0
    y, bnd = ref
    err = (got.double() - y).abs()
    assert bool(torch.isfinite(err).all()), "non-finite output"
    ratio = err / bnd
    worst = float(ratio.max())
    assert worst <= 1, f"{int((ratio > 1).sum())} outputs past the bound; first at {tuple(int(v) for v in (ratio > 1).nonzero()[0])}"
    return worst


def check_silu(got, pre, res=None):
    """exact regime of a SiLU layer: got against the float64 pre-activation (+ the residual values) by the either-neighbour rule --
    every element equals the RNE rounding of the float64 SiLU, or, where that SiLU lies within the kernels' error of a rounding
    midpoint (`near`), the result of the other bf16 neighbour.  -> the share of `near` elements"""
    from tests import conv_contract as cc

    t, other, near = cc.silu_rounding(pre)
    want = cc.epilogue(pre, 2, res, t).to(torch.bfloat16).view(torch.int16)
    alt = cc.epilogue(pre, 2, res, other).to(torch.bfloat16).view(torch.int16)
    gi = got.contiguous().view(torch.int16)
    bad = (gi != want) & ~(near & (gi == alt))
    nbad = int(bad.sum())
    assert not nbad, f"{nbad} of {bad.numel()} outputs differ; first at {tuple(int(v) for v in bad.nonzero()[0])}"
    return float(near.double().mean())


# ---------------------------------------------------------------------------------------------------------------------------------
# md_c3_pair: the draws of test_c3pair_gpu.py (test_conv_reference_cpu.py checks the exact draw's conditions on the same values)
# ---------------------------------------------------------------------------------------------------------------------------------
def c3_pair_seed(case, exact):
    return 4000 + 2 * (len(case[0]) * 7 + case[2]) + int(exact)


def c3_pair_operands(case, exact, device):
    """one regime's draw of a row of test_c3pair_gpu.CASES -> (x, w1l, b1, w2l, b2): x [N, H, W, XC] bf16 with NaN in every channel
    the call must not read, logical weights w1l [C, C] and w2l [C, 3, 3, C] bf16, biases f32.  Drawn on the CPU generator whatever the
    device, so the conditions conv_contract.reference_c3_pair asserts can be checked without a GPU on the very values the GPU test uses.

    The exact draw keeps a chain of two SiLU layers exact: x in {-1, 0, 1}; every row of w1 has 6 non-zeros of +-1/2 and b1 is one of
    0.5, 1.0 .. 3.0, so the stage-1 pre-activation takes 18 values in [-2.5, 6], none of them near a rounding midpoint of SiLU, and t
    has a smallest quantum of 2^-10; w2 is +-2^-2 (C = 32) or +-2^-3 (C = 64, 128) at density 1/3 and b2 an integer |b2| <= 3: the
    stage-2 pre-activation has a standard deviation of 3 to 6 and reaches +-20, so SiLU is exercised from its flat tail to its linear
    branch, and stage 2 needs 18 to 20 of fp32's 24 bits."""
    name, n, h, w, c, shortcut, passt, xc, xo = case[:9]
    g = torch.Generator().manual_seed(c3_pair_seed(case, exact))
    if exact:
        x = torch.randint(-1, 2, (n, h, w, xc), generator=g).to(torch.bfloat16)
        cols = torch.rand((c, c), generator=g).argsort(dim=1)[:, :6]
        w1l = torch.zeros((c, c)).scatter_(1, cols, torch.randint(0, 2, (c, 6), generator=g).float() - 0.5).to(torch.bfloat16)
        b1 = torch.randint(1, 7, (c,), generator=g).float() * 0.5
        sign = torch.randint(0, 2, (c, 3, 3, c), generator=g).float() * 2 - 1
        w2l = (sign * (torch.rand((c, 3, 3, c), generator=g) < 1 / 3) * (0.25 if c == 32 else 0.125)).to(torch.bfloat16)
        b2 = torch.randint(-3, 4, (c,), generator=g).float()
    else:
        d = Data(False, c3_pair_seed(case, exact), "cpu")
        x, w1l, b1 = d.act((n, h, w, xc)), d.weight((c, c), c), d.bias(c, c)
        w2l, b2 = d.weight((c, 3, 3, c), 9 * c), d.bias(c, c)
    read = torch.zeros(xc, dtype=torch.bool)
    read[xo:xo + (2 * c if passt else c)] = True
    x[..., ~read] = float("nan")
    return tuple(v.to(device) for v in (x, w1l, b1, w2l, b2))


# ---------------------------------------------------------------------------------------------------------------------------------
# md_conv2d_grouped: the cases of test_centerpoint_conv_gpu.py (test_conv_reference_cpu.py plants its defects in one of them)
# ---------------------------------------------------------------------------------------------------------------------------------
# the 36 branches of the nuScenes CenterHead: per task reg 2, height 1, dim 3, rot 2, vel 2, hm 1 | 2
REAL_COUTS = [c for nc in (1, 2, 2, 1, 2, 2) for c in (2, 1, 3, 2, 2, nc)]


def _odd_reversed_offsets(couts):
    """the groups' outputs in reverse order, each from an odd channel, at least one unwritten channel between two groups"""
    offs, off = [0] * len(couts), 1
    for g in reversed(range(len(couts))):
        offs[g] = off
        off += couts[g] + 1
        off += 1 - off % 2
    return offs, (off + 7) // 8 * 8


def _scattered_rows(couts):
    """w_row of each group: the groups in reverse order with a three-row gap in front of each"""
    rows, r = [0] * len(couts), 0
    for g in reversed(range(len(couts))):
        rows[g] = r + 3
        r += 3 + couts[g]
    return rows


_EVERY = list(range(1, 17))
_EVERY_OFFS, _EVERY_CY = _odd_reversed_offsets(_EVERY)
# name: (N, H, W), couts, k, relu, and optionally x_c_off, extra_c (channels of x behind the last group), y_offs, Cy, w_rows.
# The kernel's tile is 8 x 32 pixels, a work item one (tile, group) pair; workgroups come in eights (one per XCD).
GROUPED_CASES = {
    "one_tile": dict(nhw=(1, 8, 32), couts=[16], k=3, relu=0),                                        # n_work 1: seven workgroups exit
    "one_pixel_over": dict(nhw=(1, 9, 33), couts=[1, 2, 3], k=3, relu=1),
    "sub_tile_k3": dict(nhw=(1, 5, 3), couts=[4, 1], k=3, relu=0),                                    # n_work 2
    "sub_tile_k1": dict(nhw=(1, 5, 3), couts=[4, 1], k=1, relu=0),
    "ragged": dict(nhw=(3, 17, 65), couts=[3, 1, 2, 16, 5], k=3, relu=0, x_c_off=136, extra_c=24),     # n_work 135 = 8 x 16 + 7
    "every_cout": dict(nhw=(1, 12, 33), couts=_EVERY, k=3, relu=0, y_offs=_EVERY_OFFS, Cy=_EVERY_CY, w_rows=_scattered_rows(_EVERY)),
    "max_groups": dict(nhw=(1, 8, 32), couts=[g % 16 + 1 for g in range(64)], k=3, relu=0),
    "real_head": dict(nhw=(2, 19, 37), couts=REAL_COUTS, k=3, relu=0, Cy=72),
    "k1_ragged": dict(nhw=(2, 19, 37), couts=[3, 1, 16, 2], k=1, relu=0, y_offs=[0, 30, 8, 26], Cy=32),
    "k1_ragged_relu": dict(nhw=(2, 19, 37), couts=[3, 1, 16, 2], k=1, relu=1, y_offs=[0, 30, 8, 26], Cy=32),
}


def grouped_seed(name, exact):
    return 3000 + 2 * list(GROUPED_CASES).index(name) + int(exact)


def grouped_operands(name, exact, device):
    """one regime's draw of a case -> (x, wls, biases, attrs dict, y_shape): logical weights [cout_g, k, k, 64] bf16, biases f32"""
    from tests import conv_contract as cc

    c = GROUPED_CASES[name]
    d = Data(exact, grouped_seed(name, exact), device)
    n, h, w = c["nhw"]
    couts, k = c["couts"], c["k"]
    a = cc.grouped_attrs(k, couts, c.get("y_offs"), c.get("w_rows"), c["relu"], c.get("x_c_off", 0))
    x = d.act((n, h, w, a["x_c_off"] + 64 * len(couts) + c.get("extra_c", 0)))
    wls = [d.weight((co, k, k, 64), 64 * k * k) for co in couts]
    biases = [d.bias(co, co) for co in couts]
    return x, wls, biases, a, (n, h, w, c.get("Cy", (sum(couts) + 7) // 8 * 8))
