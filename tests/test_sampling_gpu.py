"""-m gpu: the two kernels that sample an image at floating-point coordinates, md_deform_cols (DCNv2 im2col) and md_image_preprocess
(affine warp + normalisation), called through the C ABI with the attribute structs nn_ops builds, and compared over the WHOLE output
with the float64 references of tests/sample_contract.py (which derives every bound; tests/test_sample_reference_cpu.py judges those
references against float64 grid_sample, fp32 emulations and planted faults).

Every output lives inside a bf16-NaN sentinel buffer with guard zones (test_conv_production_gpu's _sentinel_out / _check_guards): no
sentinel may be left in the output and the guards stay intact.  x, off and the uint8 image sit between guards too (NaN for bf16, 255
for uint8, with an all-zero image in one case), so a read outside an input shows in the output.  sample_contract.check must report
zero bad elements: bit for bit where the reference's error term is 0 (the whole exact regime), within e + half a bf16 ulp elsewhere.
Each case prints its worst err / bound and the largest share of the fp32 term e it needs (`pytest -s`).

md_deform_cols: small cases (N, H, W) x C x (k, stride, pad) x Coff (3 k k, and rounded up to 8 with NaN in the extra channels) x
regime (exact: integers, quarter offsets, masks exactly 0, 1/2, 1; gaussian: N(0, 1) data, N(0, 1.5^2) offsets and N(0, 2^2) logits
with draws over every bf16 value, +-inf and NaN), coordinates planted exactly on -1, 0, H - 1, H, W, -1/4, H - 3/4 and W - 1/4 in
every case; the three CenterNet-R18 neck layers at 512 x 512, batch 2.  Then the DCN module chain at those three shapes stage by stage:
the offset conv against conv_contract.conv_stage, md_deform_cols fed the device offsets against sample_contract, the 1 x 1 GEMM fed the
device columns against conv_contract.conv_stage (K = 9 C) -- and nn_ops.deform_conv2d gives the bit-identical result.

md_image_preprocess: a [3, 37, 53, 3] source into 32 x 64 in four layouts with one matrix per image (identity, integer and quarter-pixel
translations, 90-degree rotations and the transpose, 30-degree rotations with scale, scale 0.37, translation 1e6, entries 1e30 and
+-inf), a constant-255 and an all-zero image; [2, 480, 640, 3] -> 512 x 512 in both production layouts with get_affine_transform's
matrix, plain and composed with a 10-degree rotation."""
import pytest
import torch

from minddet_amd import _lib, nn_ops
from tests import conv_contract as cc
from tests import sample_contract as sc
from tests.conftest import has_gpu
from tests.test_conv_production_gpu import GUARD, SENTINEL, _check_guards, _sentinel_out

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"


def _guarded_bf16(t):
    """t (bf16) copied into the middle of a NaN-sentinel buffer -> (view, flat)"""
    v, flat = _sentinel_out(tuple(t.shape))
    v.copy_(t)
    return v, flat


def _guarded_u8(t):
    flat = torch.full((t.numel() + 2 * GUARD,), 255, dtype=torch.uint8, device=DEV)
    v = flat[GUARD:GUARD + t.numel()].view(t.shape)
    v.copy_(t)
    return v, flat


def _judge(what, got, flat, ref):
    _check_guards(flat)
    assert not bool((got.view(torch.int16) == SENTINEL).any()), f"{what}: output element left unwritten"
    nb, worst, first = sc.check(got, *ref)
    print(f"worst err/bound {what}: {worst:.4f}, share of e used {sc.e_share(got, *ref[:2]):.4f}")
    assert nb == 0, f"{what}: {nb} of {got.numel()} elements outside the contract; first at {first}: got {got[first].item()}, want " \
                    f"{ref[0][first].item()} +- {ref[1][first].item()}"
    return worst


def _deform_cols(x, off, k, s, p):
    """md_deform_cols on guarded copies of x and off -> (cols, its sentinel buffer)"""
    n, h, w, c = x.shape
    xg, xflat = _guarded_bf16(x)
    og, oflat = _guarded_bf16(off)
    cols, flat = _sentinel_out((n, off.shape[1], off.shape[2], k * k * c))
    _lib.call("md_deform_cols", [xg, og, cols], extra=nn_ops._PoolAttrs3(k, s, p, 0))
    torch.cuda.synchronize()
    _check_guards(xflat)
    _check_guards(oflat)
    return cols, flat


@pytest.mark.parametrize("ksp", sc.DCN_SMALL_KSP, ids=lambda v: "k%d_s%d_p%d" % v)
@pytest.mark.parametrize("C", sc.DCN_SMALL_C)
@pytest.mark.parametrize("shape", sc.DCN_SMALL_SHAPES, ids=lambda v: "%dx%dx%d" % v)
def test_deform_cols_small(shape, C, ksp):
    cases = [c for c in sc.dcn_small_cases() if c[:3] == (shape, C, ksp)]
    assert len(cases) == 4
    for (_, _, (k, s, p), padded, exact, seed) in cases:
        x, off, _ = sc.gen_dcn(shape, C, k, s, p, padded, exact, seed, DEV)
        cols, flat = _deform_cols(x, off, k, s, p)
        v, e, fill = sc.deform_cols(x, off, k, s, p)
        if exact:
            assert bool((e[~torch.isnan(v)] == 0).all())          # the whole case is judged bit for bit
        _judge(f"md_deform_cols {shape} C{C} k{k} s{s} p{p} Coff{off.shape[3]} {'exact' if exact else 'gaussian'}", cols, flat, (v, e, fill))


@pytest.mark.parametrize("shape", sc.DCN_PRODUCTION, ids=lambda v: "%dx%dx%dx%d" % v)
def test_deform_cols_production(shape):
    n, h, w, c = shape
    x, off, _ = sc.gen_dcn((n, h, w), c, 3, 1, 1, True, False, 900 + h, DEV)
    cols, flat = _deform_cols(x, off, 3, 1, 1)
    _judge(f"md_deform_cols production {shape} gaussian", cols, flat, sc.deform_cols(x, off, 3, 1, 1))


def _bounded(what, got, y, bnd):
    err = (got.double() - y).abs()
    assert bool(torch.isfinite(err).all()), f"{what}: non-finite output"
    worst = float((err / bnd).max())
    print(f"worst err/bound {what}: {worst:.4f}")
    assert worst <= 1, f"{what}: {int((err > bnd).sum())} outputs past the bound"


@pytest.mark.parametrize("shape", sc.DCN_PRODUCTION, ids=lambda v: "%dx%dx%dx%d" % v)
def test_deform_conv_chain_by_stage(shape):
    from minddet_amd import graphs

    n, h, w, c = shape
    cout = c // 2
    m = graphs.DeformConvModule(graphs.ParamInit(5 + h), c, cout, 3, 1, 1).to(DEV)
    po, pc = m.packed_offset, m.packed
    assert po.korder == 0 and pc.korder == 0 and po.cout == sc.coff_of(3, True) and pc.cout == cout and pc.relu == 1
    g = torch.Generator(device=DEV).manual_seed(h)
    x = torch.randn(shape, generator=g, device=DEV).to(torch.bfloat16)
    # (a) the offset conv
    off, oflat = _sentinel_out((n, h, w, po.cout))
    nn_ops.conv2d(x, po, out=off)
    torch.cuda.synchronize()
    _check_guards(oflat)
    wl = po.w[:po.cout, :9 * c].reshape(po.cout, 3, 3, c)
    y, bnd = cc.conv_stage(x, 0.0, wl, po.bias[:po.cout], cc._plain(n, h, w, c, 3, 1, 1, po.cout), 0)
    _bounded(f"chain {shape} (a) offset conv", off, y, bnd)
    # (b) md_deform_cols on the device offsets
    cols, flat = _deform_cols(x, off, 3, 1, 1)
    _judge(f"chain {shape} (b) md_deform_cols", cols, flat, sc.deform_cols(x, off, 3, 1, 1))
    # (c) the 1 x 1 GEMM over the device columns, K = 9 C
    pw = nn_ops.PackedConv(pc.w, pc.bias, 9 * c, pc.cout, 1, 1, 1, 0, pc.relu)
    pw.cin_real, pw.korder = 9 * c, 0
    out, yflat = _sentinel_out((n, h, w, cout))
    nn_ops.conv2d(cols, pw, out=out)
    torch.cuda.synchronize()
    _check_guards(yflat)
    wl2 = pc.w[:cout, :9 * c].reshape(cout, 1, 1, 9 * c)
    y, bnd = cc.conv_stage(cols, 0.0, wl2, pc.bias[:cout], cc._plain(n, h, w, 9 * c, 1, 1, 0, cout), pc.relu)
    _bounded(f"chain {shape} (c) GEMM", out, y, bnd)
    whole = nn_ops.deform_conv2d(x, po, pc)
    assert torch.equal(whole.view(torch.int16), out.view(torch.int16)), "nn_ops.deform_conv2d differs from its three calls"


def _preprocess(img, mat, hw, lo, hi, C):
    ig, iflat = _guarded_u8(img)
    out, flat = _sentinel_out((img.shape[0], hw[0] + lo + hi, hw[1] + lo + hi, C))
    _lib.call("md_image_preprocess", [ig, mat.to(DEV), sc.norm_tensor(DEV), out], extra=nn_ops._PreAttrs(hw[0], hw[1], lo, hi))
    torch.cuda.synchronize()
    assert bool((iflat[:GUARD] == 255).all()) and bool((iflat[-GUARD:] == 255).all())
    return out, flat


@pytest.mark.parametrize("layout,name,kind", sc.warp_small_cases(), ids=lambda v: str(v))
def test_image_preprocess_small(layout, name, kind):
    C, lo, hi = sc.WARP_LAYOUTS[layout]
    img = sc.gen_image(kind, sc.WARP_SRC, 5, DEV)
    mat = sc.warp_matrix_sets()[name]
    out, flat = _preprocess(img, mat, sc.WARP_OUT, lo, hi, C)
    ref = sc.image_preprocess(img, mat, sc.norm_tensor(), sc.WARP_OUT, lo, hi, C)
    _judge(f"md_image_preprocess {layout} {name} {kind}", out, flat, ref)


@pytest.mark.parametrize("rot", [0, 10])
@pytest.mark.parametrize("layout", ["stem", "c8"])
def test_image_preprocess_production(layout, rot):
    C, lo, hi = sc.WARP_LAYOUTS[layout]
    assert (lo, hi) == ((nn_ops.STEM_PAD_LO, nn_ops.STEM_PAD_HI) if layout == "stem" else (0, 0))
    img = sc.gen_image("random", (2, 480, 640), 11, DEV)
    mat = sc.production_warp_matrices(rot)
    out, flat = _preprocess(img, mat, (512, 512), lo, hi, C)
    ref = sc.image_preprocess(img, mat, sc.norm_tensor(), (512, 512), lo, hi, C)
    _judge(f"md_image_preprocess production {layout} rot {rot}", out, flat, ref)
