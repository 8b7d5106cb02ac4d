"""No GPU: the float64 references of tests/sample_contract.py (md_deform_cols, md_image_preprocess) judged four ways.

* An independent statement of the sampling rule: float64 torch.nn.functional.grid_sample(mode='bilinear', padding_mode='zeros',
  align_corners=True) with coordinates mapped by 2 p / (size - 1) - 1.  Both references' sampling stages must agree with it to 1e-12
  of the image's scale on the edge-planted inputs (non-finite coordinates excluded: grid_sample has no rule for them).
* The existing numpy oracle (oracle/np_ops.py::image_preprocess, fp32) lies within the derived fp32 bound on the inputs of
  tests/test_preprocess_gpu.py.
* An fp32 numpy emulation of each kernel -- the operation order of the .hip source, float32 throughout, once with separate multiply /
  add and once with every a * b + c fused (float64 product and sum, rounded once) -- passes sample_contract.check on every case of
  tests/test_sampling_gpu.py; the worst err / bound of each case is printed (`pytest -s`).
* The same emulation with one fault planted (FAULTS_DCN, FAULTS_WARP) fails check on at least one small case.

And the channel order: the reshape / transpose / concat chain of the reference wrapper (ModulatedDeformConv2d.construct) restated on
a tensor of channel labels hands the primitive (dx of taps 0..8, dy of taps 0..8, mask of taps 0..8) = the header's 2t = dy,
2t + 1 = dx, 18 + t = mask."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import np_ops
from tests import sample_contract as sc

f32 = np.float32
LOG2E = f32(1.4426950408889634)


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _mad(a, b, c, fma):
    return _fma(a, b, c) if fma else (a * b).astype(f32) + c


def _bf16_round(a):
    return torch.from_numpy(a).to(torch.bfloat16).float().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 emulations (csrc/dcn.hip deform_cols_kernel, csrc/preproc.hip image_preprocess_kernel), with planted faults
# ---------------------------------------------------------------------------------------------------------------------------------
FAULTS_DCN = ("swap_dy_dx", "tap_index", "mask_next_tap", "trunc", "drop_partial", "le_h_minus_1", "coff_3kk", "batch_offset",
              "stride_ignored", "k_order", "mask_before_rounding")
FAULTS_WARP = ("swap_m1_m3", "swap_m2_m5", "trunc", "clamp_to_edge", "pad_lo_one_axis", "channel3", "norm_by_parity", "inv256",
               "matrix_batch")


def emu_dcn(x, off, k, stride, pad, fma=False, fault=None):
    xs = x.float().numpy()
    N, H, W, C = xs.shape
    _, Ho, Wo, Coff = off.shape
    Tn = k * k
    flat = off.float().numpy().reshape(-1)
    pix = np.arange(N * Ho * Wo)
    cf = 3 * Tn if fault == "coff_3kk" else Coff
    t = np.arange(Tn)
    o = lambda c: flat[pix[:, None] * cf + c[None, :]]
    dy, dx = o(2 * t), o(2 * t + 1)
    if fault == "swap_dy_dx":
        dy, dx = dx, dy
    l = o(2 * Tn + ((t + 1) % Tn if fault == "mask_next_tap" else t))
    with np.errstate(all="ignore"):
        m = f32(1) / (f32(1) + np.exp2((-l * LOG2E).astype(f32)).astype(f32))
    ky, kx = (t % k, t // k) if fault == "tap_index" else (t // k, t % k)
    s = 1 if fault == "stride_ignored" else stride
    wo, ho, n = pix % Wo, (pix // Wo) % Ho, pix // (Wo * Ho)
    if fault == "batch_offset":
        n = np.zeros_like(n)
    with np.errstate(all="ignore"):
        y = (ho[:, None] * s - pad + ky[None, :]).astype(f32) + dy
        xx = (wo[:, None] * s - pad + kx[None, :]).astype(f32) + dx
        if fault == "drop_partial":
            ok = (y >= 0) & (y < H) & (xx >= 0) & (xx < W)
        elif fault == "le_h_minus_1":
            ok = (y > -1) & (y <= H - 1) & (xx > -1) & (xx <= W - 1)
        else:
            ok = (y > -1) & (y < H) & (xx > -1) & (xx < W)
    y, xx = np.where(ok, y, f32(0)), np.where(ok, xx, f32(0))
    yf, xf = (np.trunc(y), np.trunc(xx)) if fault == "trunc" else (np.floor(y), np.floor(xx))
    y0, x0 = yf.astype(np.int64), xf.astype(np.int64)
    ly, lx = y - yf, xx - xf
    hy, hx = f32(1) - ly, f32(1) - lx
    acc = np.zeros((pix.size, Tn, C), f32)
    for q in range(4):
        yy, xq = y0 + (q >> 1), x0 + (q & 1)
        w = ((ly if q >> 1 else hy) * (lx if q & 1 else hx)).astype(f32)
        inb = ok & (yy >= 0) & (yy < H) & (xq >= 0) & (xq < W)
        px = xs[n[:, None], yy.clip(0, H - 1), xq.clip(0, W - 1)]
        acc = np.where(inb[..., None], _mad(np.broadcast_to(w[..., None], px.shape), px, acc, fma), acc)
    if fault == "mask_before_rounding":
        acc = _bf16_round(acc)
    with np.errstate(invalid="ignore"):
        col = (acc * m[..., None]).astype(f32)
    if fault == "k_order":
        col = col.transpose(0, 2, 1)
    return torch.from_numpy(np.ascontiguousarray(col).reshape(N, Ho, Wo, Tn * C)).to(torch.bfloat16)


def emu_warp(img, mat, norm, out_hw, pad_lo, pad_hi, C, fma=False, fault=None):
    im = img.numpy()
    N, Hs, Ws, _ = im.shape
    ho, wo = out_hw
    Hp, Wp = ho + pad_lo + pad_hi, wo + pad_lo + pad_hi
    m = mat.numpy().astype(f32)
    nm = norm.numpy().astype(f32)
    out = np.zeros((N, Hp, Wp, C), f32)
    yp, xp = np.meshgrid(np.arange(Hp), np.arange(Wp), indexing="ij")
    xi, yi = xp - pad_lo, yp - (0 if fault == "pad_lo_one_axis" else pad_lo)
    inside = (xi >= 0) & (xi < wo) & (yi >= 0) & (yi < ho)
    xq, yq = xi.astype(f32), yi.astype(f32)
    inv = f32(1) / f32(256 if fault == "inv256" else 255)
    for b in range(N):
        mm = m[0 if fault == "matrix_batch" else b].copy()
        if fault == "swap_m1_m3":
            mm[[1, 3]] = mm[[3, 1]]
        if fault == "swap_m2_m5":
            mm[[2, 5]] = mm[[5, 2]]
        with np.errstate(all="ignore"):
            sx = _mad(np.full_like(xq, mm[1]), yq, (mm[0] * xq).astype(f32), fma) + mm[2]
            sy = _mad(np.full_like(xq, mm[4]), yq, (mm[3] * xq).astype(f32), fma) + mm[5]
            ok = (sx > -1) & (sx < Ws) & (sy > -1) & (sy < Hs)
        sx, sy = np.where(ok, sx, f32(0)), np.where(ok, sy, f32(0))
        xf, yf = (np.trunc(sx), np.trunc(sy)) if fault == "trunc" else (np.floor(sx), np.floor(sy))
        x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
        lx, ly = sx - xf, sy - yf
        v = np.zeros((Hp, Wp, 3), f32)
        for q in range(4):
            yy, xx = y0 + (q >> 1), x0 + (q & 1)
            w = ((ly if q >> 1 else f32(1) - ly) * (lx if q & 1 else f32(1) - lx)).astype(f32)
            inb = ok & ((yy >= 0) & (yy < Hs) & (xx >= 0) & (xx < Ws) if fault != "clamp_to_edge" else True)
            px = im[b, yy.clip(0, Hs - 1), xx.clip(0, Ws - 1)].astype(f32)
            v = np.where(inb[..., None], _mad(np.broadcast_to(w[..., None], px.shape), px, v, fma), v)
        if fault == "norm_by_parity":
            par = (xi & 1)[..., None] + np.zeros(3, np.int64)
            mean, std = nm[par], nm[3 + par]
        else:
            mean, std = nm[:3], nm[3:]
        v = ((_mad(v, np.full_like(v, inv), -np.broadcast_to(mean, v.shape), fma) if fma else (v * inv).astype(f32) - mean) / std).astype(f32)
        out[b, ..., :3] = np.where(inside[..., None], v, f32(0))
        if fault == "channel3":
            out[b, ..., 3] = out[b, ..., 0]
    return torch.from_numpy(out).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------------------------
# cases (those of tests/test_sampling_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
DCN_SMALL = sc.dcn_small_cases()
_cache = {}


def _dcn_case(case):
    """(x, off, plants, v, e, fill), computed once per case"""
    if case not in _cache:
        shape, C, (k, s, p), padded, exact, seed = case
        x, off, plants = sc.gen_dcn(shape, C, k, s, p, padded, exact, seed, "cpu")
        _cache[case] = (x, off, plants) + sc.deform_cols(x, off, k, s, p)
    return _cache[case]


WARP_SMALL = sc.warp_small_cases()


def _warp_case(case):
    if case not in _cache:
        layout, name, kind = case
        C, lo, hi = sc.WARP_LAYOUTS[layout]
        img = sc.gen_image(kind, sc.WARP_SRC, 5, "cpu")
        mat = sc.warp_matrix_sets()[name]
        _cache[case] = (img, mat, lo, hi, C) + sc.image_preprocess(img, mat, sc.norm_tensor(), sc.WARP_OUT, lo, hi, C)
    return _cache[case]


# ---------------------------------------------------------------------------------------------------------------------------------
# the independent judge
# ---------------------------------------------------------------------------------------------------------------------------------
def _grid_sample(img_nhwc, y, x):
    """float64 grid_sample of img [N, H, W, C] at (y, x) [N, P] -> [N, P, C]"""
    N, H, W, C = img_nhwc.shape
    grid = torch.stack([2 * x / (W - 1) - 1, 2 * y / (H - 1) - 1], -1).view(N, 1, -1, 2)
    out = F.grid_sample(img_nhwc.permute(0, 3, 1, 2).contiguous(), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    return out[:, :, 0].permute(0, 2, 1)


@pytest.mark.parametrize("case", [c for c in DCN_SMALL if c[1] == 8], ids=str)
def test_dcn_sampling_vs_grid_sample(case):
    shape, C, (k, s, p), padded, exact, seed = case
    x, off = _dcn_case(case)[:2]
    N, H, W = shape
    y, xx, _ = sc.dcn_coords(off, H, W, k, s, p)
    smp, _ = sc.deform_samples(x, off, k, s, p)
    fin = torch.isfinite(y) & torch.isfinite(xx)
    z = torch.zeros_like(y)
    ref = _grid_sample(x.double(), torch.where(fin, y, z).reshape(N, -1), torch.where(fin, xx, z).reshape(N, -1)).reshape(smp.v.shape)
    err = (smp.v - ref).abs()[fin]
    assert fin.float().mean() > 0.8 and float(err.max()) <= 1e-12 * float(x.double().abs().max())


@pytest.mark.parametrize("name", list(sc.warp_matrix_sets()))
@pytest.mark.parametrize("kind", ["random", "white"])
def test_warp_sampling_vs_grid_sample(name, kind):
    img = sc.gen_image(kind, sc.WARP_SRC, 5, "cpu")
    mat = sc.warp_matrix_sets()[name]
    N = img.shape[0]
    sx, sy = sc.warp_coords(mat, sc.WARP_OUT, "cpu")
    smp = sc.warp_samples(img, mat, sc.WARP_OUT)
    fin = torch.isfinite(sx.v) & torch.isfinite(sy.v)
    z = torch.zeros_like(sx.v)
    ref = _grid_sample(img.double(), torch.where(fin, sy.v, z).reshape(N, -1), torch.where(fin, sx.v, z).reshape(N, -1)).reshape(smp.v.shape)
    err = (smp.v - ref).abs()[fin]
    assert float(err.max()) <= 1e-12 * 255.0
    assert bool((smp.v[~fin] == 0).all())


def test_edge_plants_land_on_their_targets():
    for case in DCN_SMALL:
        shape, C, (k, s, p), padded, exact, seed = case
        _, off, plants = _dcn_case(case)[:3]
        _, H, W = shape
        y, x, l = sc.dcn_coords(off, H, W, k, s, p)
        want = set(sc.edge_targets(H, W))
        for (n, ho, wo, t, py, px) in plants["edges"]:
            assert float(y[n, ho, wo, t]) == py and float(x[n, ho, wo, t]) == px
            want -= {(0, py), (1, px)}
        assert not want and len({q[:4] for q in plants["edges"]}) == len(plants["edges"])
        assert bool(torch.isnan(off[..., 3 * k * k:].float()).all())
        if not exact:
            assert len(plants["nonfinite"]) == len(sc.NONFINITE_PLANTS)
        else:
            d = off[..., :2 * k * k].float()
            assert float(d[..., 0::2].mean()) > 0 > float(d[..., 1::2].mean())      # dy and dx drawn differently


def test_exact_regime_has_no_error_term():
    for case in DCN_SMALL:
        if case[4]:
            v, e = _dcn_case(case)[3:5]
            assert bool((e[~torch.isnan(v)] == 0).all())
    for name in ("identity_shift", "quarter", "rot90_transpose"):
        img = sc.gen_image("random", sc.WARP_SRC, 5, "cpu")
        assert bool((sc.warp_samples(img, sc.warp_matrix_sets()[name], sc.WARP_OUT).e == 0).all())      # e from the normalisation only


# ---------------------------------------------------------------------------------------------------------------------------------
# the existing oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def test_warp_reference_vs_numpy_oracle():
    """the inputs of tests/test_preprocess_gpu.py::test_affine_warp_vs_oracle and ::test_identity_matrix_is_exact_normalisation"""
    from minddet_amd import det_ops

    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (3, 120, 200, 3), dtype=np.uint8)
    mats = [np.asarray(det_ops.get_affine_transform(np.array([100.0 + 7 * b, 60.0 - 3 * b], np.float32), 210.0 + 15 * b, (128, 64), inv=True),
                       np.float32).reshape(6) for b in range(3)]
    img0 = np.random.default_rng(0).integers(0, 256, (2, 32, 64, 3), dtype=np.uint8)
    ident = np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32), (2, 1))
    for im, mat, hw in ((img, np.stack(mats), (64, 128)), (img0, ident, (32, 64))):
        ref = np_ops.image_preprocess(im, mat, sc.MEAN, sc.STD, hw)
        v, e, _ = sc.image_preprocess(torch.from_numpy(im), torch.from_numpy(mat), sc.norm_tensor(), hw, 0, 0, 4)
        err = (torch.from_numpy(ref).double() - v[..., :3]).abs()
        assert bool((err <= e[..., :3]).all()), float((err - e[..., :3]).max())
        print(f"numpy oracle vs reference {hw}: worst err / e {float((err / e[..., :3].clamp(min=1e-300)).max()):.3f}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the bound holds for the fp32 emulations, and planted faults break it
# ---------------------------------------------------------------------------------------------------------------------------------
def _ratio_dcn(x, off, k, s, p, ref, **kw):
    return sc.check(emu_dcn(x, off, k, s, p, **kw), *ref)


@pytest.mark.parametrize("case", DCN_SMALL, ids=str)
def test_dcn_emulation_inside_bound(case):
    shape, C, (k, s, p), padded, exact, seed = case
    x, off, _, v, e, fill = _dcn_case(case)
    for fma in (False, True):
        got = emu_dcn(x, off, k, s, p, fma=fma)
        nb, worst, first = sc.check(got, v, e, fill)
        print(f"dcn {case} fma={int(fma)}: worst err/bound {worst:.4f}, share of e used {sc.e_share(got, v, e):.4f}")
        assert nb == 0 and worst <= 1, (nb, worst, first)


@pytest.mark.parametrize("shape", sc.DCN_PRODUCTION, ids=str)
def test_dcn_emulation_inside_bound_production(shape):
    N, H, W, C = shape
    x, off, _ = sc.gen_dcn((N, H, W), C, 3, 1, 1, True, False, 900 + H, "cpu")
    ref = sc.deform_cols(x, off, 3, 1, 1)
    for fma in (False, True):
        got = emu_dcn(x, off, 3, 1, 1, fma=fma)
        nb, worst, first = sc.check(got, *ref)
        print(f"dcn production {shape} fma={int(fma)}: worst err/bound {worst:.4f}, share of e used {sc.e_share(got, *ref[:2]):.4f}")
        assert nb == 0 and worst <= 1, (nb, worst, first)


@pytest.mark.parametrize("fault", FAULTS_DCN)
def test_dcn_planted_fault_fails(fault):
    failed = []
    for case in DCN_SMALL:
        shape, C, (k, s, p), padded, exact, seed = case
        if C != 8 or (fault == "coff_3kk" and not padded):
            continue
        x, off, _, v, e, fill = _dcn_case(case)
        if _ratio_dcn(x, off, k, s, p, (v, e, fill), fault=fault)[0]:
            failed.append(case)
    assert failed, f"fault {fault} survives every small case"
    print(f"dcn fault {fault}: caught by {len(failed)} small cases")


@pytest.mark.parametrize("case", WARP_SMALL, ids=str)
def test_warp_emulation_inside_bound(case):
    img, mat, lo, hi, C, v, e, fill = _warp_case(case)
    for fma in (False, True):
        got = emu_warp(img, mat, sc.norm_tensor(), sc.WARP_OUT, lo, hi, C, fma=fma)
        nb, worst, first = sc.check(got, v, e, fill)
        print(f"warp {case} fma={int(fma)}: worst err/bound {worst:.4f}, share of e used {sc.e_share(got, v, e):.4f}")
        assert nb == 0 and worst <= 1, (nb, worst, first)


@pytest.mark.parametrize("layout", ["stem", "c8"])
@pytest.mark.parametrize("rot", [0, 10])
def test_warp_emulation_inside_bound_production(layout, rot):
    C, lo, hi = sc.WARP_LAYOUTS[layout]
    img = sc.gen_image("random", (2, 480, 640), 11, "cpu")
    mat = sc.production_warp_matrices(rot)
    v, e, fill = sc.image_preprocess(img, mat, sc.norm_tensor(), (512, 512), lo, hi, C)
    for fma in (False, True):
        got = emu_warp(img, mat, sc.norm_tensor(), (512, 512), lo, hi, C, fma=fma)
        nb, worst, first = sc.check(got, v, e, fill)
        print(f"warp production {layout} rot {rot} fma={int(fma)}: worst err/bound {worst:.4f}, share of e used {sc.e_share(got, v, e):.4f}")
        assert nb == 0 and worst <= 1, (nb, worst, first)


@pytest.mark.parametrize("fault", FAULTS_WARP)
def test_warp_planted_fault_fails(fault):
    failed = []
    for case in WARP_SMALL:
        img, mat, lo, hi, C, v, e, fill = _warp_case(case)
        if sc.check(emu_warp(img, mat, sc.norm_tensor(), sc.WARP_OUT, lo, hi, C, fault=fault), v, e, fill)[0]:
            failed.append(case)
    assert failed, f"fault {fault} survives every small case"
    print(f"warp fault {fault}: caught by {len(failed)} small cases")


# ---------------------------------------------------------------------------------------------------------------------------------
# channel order
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wrapper_channel_order():
    """ModulatedDeformConv2d.construct on channel labels: chunk(out, 3) -> concat(o1, o2) -> flatten -> reshape (b, 1, 3, 3, 2, h, w) ->
    transpose (0, 4, 1, 2, 3, 5, 6) -> chunk into (offsets_y1, offsets_x1); mask -> reshape (b, 1, 3, 3, 1, h, w) -> the same transpose;
    concat(offsets_x1, offsets_y1, mask) -> reshape (b, 27, h, w)"""
    b, h, w = 2, 3, 4
    out = torch.arange(27.0).view(1, 27, 1, 1).expand(b, 27, h, w).contiguous()
    o1, o2, mask = torch.chunk(out, 3, dim=1)
    ms_off = torch.cat((o1, o2), dim=1).flatten(1).reshape(b, 1, 3, 3, 2, h, w).permute(0, 4, 1, 2, 3, 5, 6)
    off_y, off_x = torch.chunk(ms_off, 2, dim=1)
    ms_mask = mask.flatten(1).reshape(b, 1, 3, 3, 1, h, w).permute(0, 4, 1, 2, 3, 5, 6)
    prim = torch.cat((off_x, off_y, ms_mask), dim=1).reshape(b, 27, h, w)
    want = [2 * t + 1 for t in range(9)] + [2 * t for t in range(9)] + [18 + t for t in range(9)]
    assert bool((prim == torch.tensor(want, dtype=torch.float32).view(1, 27, 1, 1)).all())
