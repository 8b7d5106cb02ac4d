"""-m gpu: the kernels between the conv, decode, top-k and NMS stages -- md_maxpool2d, md_sppf_pool, md_upsample_add, md_slice_cast,
md_nhwc_to_nchw_f32, md_concat_copy, md_upsample2x, md_rpn_merge, md_make_rois, md_gather_rows and md_pack_detections -- through the C
ABI, compared over the WHOLE output with the exact references of tests/move_contract.py.

Production calls: each model of tests/test_decode_production_gpu.MODELS is built at its production batch and run once the way
production runs it; a wrapper around _lib.call records every call of the eleven ops (op, shapes, attribute record).  The recorded op
set must equal the model's row of OPS (a graph change that stops calling a kernel fails here) and every distinct call is replayed on
data from the contract's generators.  md_pack_detections is replayed in as many generator phases as it takes to meet every
(num < max_det, sel_cnt >= npre, status word) combination, and once more in its 7-parameter form.

Fixed calls (FIXED): the ops the models reach only on fall-back paths (the ResNet stem's 3x3 / 2 pool in both zero_pad modes, the
unfused SPPF chain on a map md_sppf_pool_groups refuses, md_upsample_add at the FPN's P2 shape -- the FPNs of configs/ halve exactly and
take the fused conv residual instead), ragged edges (C = 8, odd sizes, a window larger than the image, tiles of the transpose that
are not full, an odd c0, size pairs that do not divide -- one of them a pair on which F.interpolate differs from the integer index
formula --, cnt NULL and given), every op with N = 0, and one call per grid-stride kernel just above 8192 x 256 work items, so that
the second trip of each loop runs whatever the production shapes become.

Checks: outputs start as a NaN sentinel between sentinel guard zones.  The guards stay intact; every element the op does not own (the
other channels of a concat / upsample destination, channels [0, C) and [4C, Ctot) of the SPPF buffer) keeps its bits; every owned
element is written and equals the reference: as bit patterns for copies, casts and the add, as numbers for the two max kernels (the
header leaves the sign of a zero maximum open).  The bf16 copies carry every one of the 65536 bit patterns, the sentinel's own among
them, so they run twice on two different fills: equal to the reference under both means written.  References are computed in
per-image chunks.  Each case prints its element count (`pytest -s`)."""
import json

import pytest
import torch

from minddet_amd import _lib, nn_ops
from tests import move_contract as mc
from tests import test_decode_production_gpu as dp
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
GUARD = 1 << 14             # sentinel elements on each side of every output
CHUNK_ELEMS = 1 << 24       # elements per reference chunk
ALT16 = 0x7FA6              # the second fill of the bf16 copy outputs
GRID_ITEMS = 8192 * 256     # work items one trip of a grid-stride kernel of pool.hip covers

MOVE_OPS = ("md_maxpool2d", "md_sppf_pool", "md_upsample_add", "md_slice_cast", "md_nhwc_to_nchw_f32", "md_concat_copy", "md_upsample2x",
            "md_rpn_merge", "md_make_rois", "md_gather_rows", "md_pack_detections")
RCNN = {"md_maxpool2d", "md_slice_cast", "md_rpn_merge", "md_make_rois", "md_pack_detections"}
YOLO = {"md_sppf_pool", "md_upsample2x", "md_gather_rows", "md_pack_detections"}
# the ops one production pass of each model calls, as recorded.  md_upsample_add is in no row: every FPN level of the 800 x 1344 input
# halves exactly, which graphs.FPN fuses into the lateral conv (FIXED replays the kernel at the P2 shape).  CenterNet takes the 8-channel
# NHWC batch, so its ResNet stem runs md_conv2d + the 3x3 / 2 zero_pad md_maxpool2d instead of md_stem_pool.  CenterPoint's
# post-processing gathers its selected boxes with md_gather_rows (cnt NULL).
OPS = {"faster_rcnn_b120": RCNN, "faster_rcnn_b60": RCNN, "mask_rcnn_b32": RCNN, "yolov5s_b32": YOLO, "yolov8l_b32": YOLO,
       "centerpoint_b4": {"md_gather_rows"}, "centernet_r18_512_b32": {"md_maxpool2d", "md_nhwc_to_nchw_f32"}}


def _struct(op, a):
    if op == "md_maxpool2d":
        return nn_ops._PoolAttrs(a["k"], a["stride"], a["pad"], a["zero_pad"])
    if op == "md_sppf_pool":
        return nn_ops._SppfAttrs(a["channels"], a["k"])
    if op == "md_upsample2x":
        return nn_ops._Upsample2xAttrs(a["c0"], a["width"], a["src_c0"])
    if op in ("md_slice_cast", "md_nhwc_to_nchw_f32", "md_concat_copy"):
        return nn_ops._SliceAttrs(a["c0"], a["width"])
    return None


def move_calls(config, batch):
    """the distinct calls (op, shapes, attrs dict) of the eleven ops in one production pass of the model"""
    m, x = dp._model_input(config, batch)
    calls, keys, orig = [], set(), _lib.call

    def record(name, tensors, extra=None, stream=None):
        if name in MOVE_OPS:
            shapes = [None if t is None else list(t.shape) for t in tensors]
            attrs = dp._fields(extra)
            key = json.dumps([name, shapes, attrs])
            if key not in keys:
                keys.add(key)
                calls.append((name, shapes, attrs))
        return orig(name, tensors, extra=extra, stream=stream)

    _lib.call = record
    try:
        getattr(m, "forward_split", m.forward)(x)
        torch.cuda.synchronize()
    finally:
        _lib.call = orig
    del m, x
    torch.cuda.empty_cache()
    return calls


# ---------------------------------------------------------------------------------------------------------------------------------
def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _out32(shape, dtype=torch.float32):
    """(tensor, flat): a 4-byte output of `shape` filled with SENT32 inside a sentinel buffer GUARD elements longer on each side"""
    n = _numel(shape)
    flat = torch.full((n + 2 * GUARD,), mc.SENT32, dtype=torch.int32, device=DEV)
    return flat[GUARD:GUARD + n].view(dtype).view(shape), flat


def _out16(shape, fill=mc.SENT16):
    """the same for a bf16 output"""
    n = _numel(shape)
    flat = torch.full((n + 2 * GUARD,), fill, dtype=torch.int16, device=DEV)
    return flat[GUARD:GUARD + n].view(torch.bfloat16).view(shape), flat


def _guards_intact(flat, fill):
    assert bool((flat[:GUARD] == fill).all()) and bool((flat[-GUARD:] == fill).all()), "write outside the output tensor"


def _chunks(n, per_image):
    nb = max(1, CHUNK_ELEMS // max(per_image, 1))
    return [(i, min(n, i + nb)) for i in range(0, n, nb)]


def _same(got, want, what):
    bad = got != want
    if bool(bad.any()):
        i = bad.flatten().nonzero()[0].item()
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements wrong; first at flat index {i}: got "
                             f"{got.flatten()[i].item()}, want {want.flatten()[i].item()}")


def _written32(t, what):
    assert not bool((mc.bits32(t) == mc.SENT32).any()), f"{what}: element left unwritten"


def _host(gen, *args, **kw):
    """an index generator run on the host (an index error in the set-up raises there), its tensors moved to the GPU"""
    ins, plants = gen(*args, "cpu", **kw)
    return [None if t is None else t.to(DEV) for t in ins], plants


def _run(op, shapes, a, seed, phase=0, status_form=None):
    """one call on generator data, checked in full; -> the number of output elements checked"""
    extra = _struct(op, a)
    if op == "md_maxpool2d":
        (x,), _ = mc.gen_pool(shapes[0], a, seed, DEV)
        y, fy = _out16(shapes[1])
        _lib.call(op, [x, y], extra=extra)
        torch.cuda.synchronize()
        _guards_intact(fy, mc.SENT16)
        assert not bool((mc.bits16(y) == mc.SENT16).any()), "element left unwritten"
        for n0, n1 in _chunks(x.shape[0], x[0].numel() if x.shape[0] else 1):
            _same(y[n0:n1].double(), mc.maxpool(x[n0:n1], a["k"], a["stride"], a["pad"], a["zero_pad"]), op)
        return y.numel()
    if op == "md_sppf_pool":
        N, H, W, Ctot = shapes[0]
        C, k = a["channels"], a["k"]
        (x,), _ = mc.gen_pool([N, H, W, C], dict(k=k, stride=1, pad=k // 2, zero_pad=0), seed, DEV, sppf_radius=k // 2)
        buf, fb = _out16(shapes[0])
        buf[..., :C] = x
        _lib.call(op, [buf], extra=extra)
        torch.cuda.synchronize()
        _guards_intact(fb, mc.SENT16)
        b = mc.bits16(buf)
        _same(b[..., :C], mc.bits16(x), "channels [0, C) (read only)")
        assert bool((b[..., 4 * C:] == mc.SENT16).all()), "write into channels [4C, Ctot)"
        assert not bool((b[..., C:4 * C] == mc.SENT16).any()), "element left unwritten"
        for n0, n1 in _chunks(N, x[0].numel() if N else 1):
            for j, want in enumerate(mc.sppf(x[n0:n1], k)):
                _same(buf[n0:n1, :, :, (j + 1) * C:(j + 2) * C].double(), want, f"{op} pool {j + 1}")
        return 3 * x.numel()
    if op == "md_upsample_add":
        (lat, top), pl = mc.gen_upsample_add(shapes, seed, DEV)
        y, fy = _out16(shapes[2])
        _lib.call(op, [lat, top, y], extra=None)
        torch.cuda.synchronize()
        _guards_intact(fy, mc.SENT16)
        yb = mc.bits16(y)
        assert not bool((yb == mc.SENT16).any()), "element left unwritten"
        nsub = 0
        for n0, n1 in _chunks(lat.shape[0], lat[0].numel() if lat.shape[0] else 1):
            want, sub = mc.upsample_add(lat[n0:n1], top[n0:n1])
            nsub += int(sub.sum())
            _same(yb[n0:n1], want, op)
        assert nsub == pl["subnormal"], f"{nsub} results below 2^-126, {pl['subnormal']} planted"
        return y.numel()
    if op in ("md_slice_cast", "md_nhwc_to_nchw_f32"):
        (x,), _ = mc.gen_patterns(shapes[0], a["c0"], a["width"], seed, DEV)
        y, fy = _out32(shapes[1])
        _lib.call(op, [x, y], extra=extra)
        torch.cuda.synchronize()
        _guards_intact(fy, mc.SENT32)
        _written32(y, op)
        ref = mc.slice_cast if op == "md_slice_cast" else mc.nhwc_to_nchw_f32
        for n0, n1 in _chunks(x.shape[0], x[0].numel() if x.shape[0] else 1):
            _same(mc.bits32(y[n0:n1]), ref(x[n0:n1], a["c0"], a["width"]), op)
        return y.numel()
    if op in ("md_concat_copy", "md_upsample2x"):
        sc0 = a.get("src_c0", 0) if op == "md_upsample2x" else 0
        (src,), _ = mc.gen_patterns(shapes[0], sc0, a["width"], seed, DEV)
        want = mc.concat_copy(src) if op == "md_concat_copy" else mc.upsample2x(src, sc0, a["width"])
        for fill in (mc.SENT16, ALT16):
            dst, fd = _out16(shapes[1], fill)
            _lib.call(op, [src, dst], extra=extra)
            torch.cuda.synchronize()
            _guards_intact(fd, fill)
            b = mc.bits16(dst)
            assert bool((b[..., :a["c0"]] == fill).all()) and bool((b[..., a["c0"] + a["width"]:] == fill).all()), \
                "write outside the destination's channel slice"
            _same(b[..., a["c0"]:a["c0"] + a["width"]], want, op)
        return want.numel()
    if op == "md_rpn_merge":
        ins, _ = _host(mc.gen_rpn_merge, shapes, seed)
        (mb, fmb), (ms, fms) = _out32(shapes[3]), _out32(shapes[4])
        _lib.call(op, ins + [mb, ms])
        torch.cuda.synchronize()
        wb, ws = mc.rpn_merge(*ins)
        for t, f, w, name in ((mb, fmb, wb, "mboxes"), (ms, fms, ws, "mscores")):
            _guards_intact(f, mc.SENT32)
            _written32(t, name)
            _same(mc.bits32(t), w, name)
        return mb.numel() + ms.numel()
    if op == "md_make_rois":
        ins, _ = _host(mc.gen_make_rois, shapes, seed)
        (rois, fr), (rs, fs) = _out32(shapes[4]), _out32(shapes[5])
        _lib.call(op, ins + [rois, rs])
        torch.cuda.synchronize()
        wr, ws = mc.make_rois(*ins)
        for t, f, w, name in ((rois, fr, wr, "rois"), (rs, fs, ws, "roi_scores")):
            _guards_intact(f, mc.SENT32)
            _written32(t, name)
            _same(mc.bits32(t), w, name)
        return rois.numel() + rs.numel()
    if op == "md_gather_rows":
        ins, _ = _host(mc.gen_gather_rows, shapes, shapes[2] is not None, seed)
        out, fo = _out32(shapes[3])
        _lib.call(op, ins + [out])
        torch.cuda.synchronize()
        _guards_intact(fo, mc.SENT32)
        _written32(out, op)
        _same(mc.bits32(out), mc.gather_rows(*ins), op)
        return out.numel()
    if op == "md_pack_detections":
        nine = len(shapes) == 9 if status_form is None else status_form
        dshape = shapes[6] if len(shapes) == 9 else shapes[5]
        B, max_det = dshape[0], dshape[1]
        ins, _ = _host(mc.gen_pack, shapes, max_det, nine, seed, phase=phase)
        (dets, fd), (count, fc) = _out32(dshape), _out32([B], torch.int32)
        if nine:
            status = ins[6].clone()
            _lib.call(op, ins[:6] + [dets, count, status])
        else:
            _lib.call(op, ins[:5] + [dets, count])
        torch.cuda.synchronize()
        wd, wc, wst = mc.pack_detections(ins[0], ins[1], ins[2], ins[3], ins[4], max_det, *(ins[5:7] if nine else ()))
        for t, f, w, name in ((dets, fd, wd, "dets"), (count, fc, wc, "count")):
            _guards_intact(f, mc.SENT32)
            _written32(t, name)
            _same(mc.bits32(t), w, name)
        if nine:
            _same(status, wst, "status")
        return dets.numel() + count.numel() + (B if nine else 0)
    raise AssertionError(op)


def _replay(case, op, shapes, a, seed):
    """one distinct call through every variant its checks need; prints the element count"""
    if op == "md_pack_detections":
        dshape = shapes[6] if len(shapes) == 9 else shapes[5]
        n = sum(_run(op, shapes, a, seed + p, phase=p, status_form=True) for p in range(mc.pack_phases(dshape[0])))
        n += _run(op, shapes, a, seed + 99, status_form=False)
    else:
        n = _run(op, shapes, a, seed)
    print(f"{case} {op} {[s for s in shapes if s is not None]} {a if a else ''}: {n} elements checked")
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case,config,batch", [m[:3] for m in dp.MODELS], ids=[m[0] for m in dp.MODELS])
def test_move_production_calls(case, config, batch):
    calls = move_calls(config, batch)
    ops = sorted({c[0] for c in calls})
    print(f"{case}: recorded ops {ops}")
    assert set(ops) == OPS[case], ops
    for j, (op, shapes, a) in enumerate(calls):
        _replay(case, op, shapes, a, 7000 + 31 * j)


# ---------------------------------------------------------------------------------------------------------------------------------
# fixed calls
# ---------------------------------------------------------------------------------------------------------------------------------
def _pool(shape, k, s, p, zp):
    n, h, w, c = shape
    return ("md_maxpool2d", [shape, [n, mc.pool_out(h, k, s, p), mc.pool_out(w, k, s, p), c]], dict(k=k, stride=s, pad=p, zero_pad=zp))


def _sppf(shape, c, k):
    return ("md_sppf_pool", [shape], dict(channels=c, k=k))


def _upadd(lat, top_hw):
    return ("md_upsample_add", [lat, [lat[0], top_hw[0], top_hw[1], lat[3]], lat], {})


def _cast(op, shape, c0, width):
    out = shape[:-1] + [width] if op == "md_slice_cast" else [shape[0], width, shape[1], shape[2]]
    return (op, [shape, out], dict(c0=c0, width=width))


def _concat(src, ctot, c0):
    return ("md_concat_copy", [src, src[:3] + [ctot]], dict(c0=c0, width=src[3]))


def _up2x(src, src_c0, width, ctot, c0):
    return ("md_upsample2x", [src, [src[0], 2 * src[1], 2 * src[2], ctot]], dict(c0=c0, width=width, src_c0=src_c0))


def _merge(L, B, k):
    return ("md_rpn_merge", [[L, B, k, 4], [L, B, k], [L, B, k], [B, L * k, 4], [B, L * k]], {})


def _rois(B, P, post):
    return ("md_make_rois", [[B, P, 4], [B, post], [B, post], [B], [B * post, 5], [B * post]], {})


def _gather(B, n, W, k, with_cnt):
    return ("md_gather_rows", [[B, n, W], [B, k], [B] if with_cnt else None, [B, k, W]], {})


def _pack(B, npre, max_det):
    return ("md_pack_detections", [[B, npre, 4], [B, npre], [B, npre], [B, npre], [B], [B], [B, max_det, 6], [B], [B]], {})


FIXED = {
    # fall-back paths of the models
    "stem_pool_zero_pad": _pool([2, 400, 672, 64], 3, 2, 1, 1),
    "stem_pool_ignore_pad": _pool([2, 400, 672, 64], 3, 2, 1, 0),
    "sppf_unfused_pool": _pool([2, 52, 52, 256], 5, 1, 2, 0),
    "sppf_unfused_concat": _concat([2, 52, 52, 256], 1024, 512),
    "fpn_p2_upsample_add": _upadd([8, 200, 336, 256], (100, 168)),
    # ragged edges
    "pool_c8_window_larger_than_image": _pool([3, 3, 5, 8], 5, 1, 2, 0),
    "pool_c8_window_larger_zero_pad": _pool([3, 3, 5, 8], 5, 1, 2, 1),
    "pool_c8_odd": _pool([2, 37, 53, 8], 3, 2, 1, 1),
    "pool_k1_s2_odd": _pool([2, 25, 43, 16], 1, 2, 0, 0),
    "pool_k7_s3": _pool([1, 20, 21, 8], 7, 3, 3, 1),
    "sppf_c8_ragged_wide_buffer": _sppf([3, 7, 9, 40], 8, 5),
    "sppf_window_larger_than_image": _sppf([2, 3, 4, 64], 16, 5),
    "sppf_k3": _sppf([2, 13, 6, 32], 8, 3),
    "sppf_40x40": _sppf([2, 40, 40, 64], 16, 5),
    "transpose_ragged": _cast("md_nhwc_to_nchw_f32", [2, 13, 7, 88], 3, 70),
    "transpose_full_tiles": _cast("md_nhwc_to_nchw_f32", [2, 64, 64, 136], 8, 128),
    "slice_cast_odd_c0": _cast("md_slice_cast", [5, 37, 24], 3, 5),
    "upsample_add_nondivisible": _upadd([2, 37, 53, 16], (19, 27)),
    "upsample_add_where_interpolate_differs": _upadd([1, 44, 46, 8], (26, 14)),
    "upsample_add_same_size": _upadd([2, 7, 9, 8], (7, 9)),
    "upsample_add_top_1x1": _upadd([2, 5, 6, 8], (1, 1)),
    "upsample2x_ragged": _up2x([2, 5, 7, 24], 8, 16, 40, 16),
    "concat_ragged": _concat([2, 5, 7, 8], 24, 8),
    "gather_rows_no_cnt": _gather(5, 50, 7, 20, False),
    "gather_rows_cnt": _gather(5, 50, 7, 20, True),
    "rpn_merge_small": _merge(3, 4, 33),
    "make_rois_small": _rois(5, 99, 17),
    "pack_small": _pack(7, 40, 9),
    "pack_max_det_above_npre": _pack(4, 6, 10),
    # N = 0
    "n0_pool": _pool([0, 9, 9, 8], 3, 2, 1, 1),
    "n0_sppf": _sppf([0, 7, 9, 32], 8, 5),
    "n0_upsample_add": _upadd([0, 8, 8, 8], (4, 4)),
    "n0_slice_cast": _cast("md_slice_cast", [0, 4, 8], 0, 4),
    "n0_transpose": _cast("md_nhwc_to_nchw_f32", [0, 4, 4, 8], 0, 4),
    "n0_concat": _concat([0, 4, 4, 8], 16, 8),
    "n0_upsample2x": _up2x([0, 4, 4, 8], 0, 8, 16, 8),
    "n0_rpn_merge": _merge(2, 0, 3),
    "n0_make_rois": _rois(0, 6, 3),
    "n0_gather_rows": _gather(0, 4, 3, 2, True),
    "n0_pack": _pack(0, 8, 5),
    # just above one trip of each grid-stride loop (POOL_GRID_CAP = 8192 workgroups of 256 lanes)
    "second_trip_maxpool": _pool([5, 128, 130, 264], 3, 1, 1, 0),
    "second_trip_upsample_add": _upadd([5, 128, 130, 264], (50, 57)),
    "second_trip_slice_cast": _cast("md_slice_cast", [1100, 64, 40], 3, 31),
    "second_trip_concat": _concat([5, 128, 130, 264], 280, 8),
    "second_trip_upsample2x": _up2x([5, 64, 65, 272], 8, 264, 280, 16),
}


def _work_items(op, shapes, a):
    """work items of the op's grid-stride loop"""
    if op == "md_slice_cast":
        return _numel(shapes[1])
    if op == "md_upsample_add":
        return _numel(shapes[2]) // 8
    if op == "md_maxpool2d":
        return _numel(shapes[1]) // 8
    return _numel(shapes[1][:3]) * a["width"] // 8


@pytest.mark.parametrize("name", list(FIXED))
def test_move_fixed_calls(name):
    op, shapes, a = FIXED[name]
    if name.startswith("second_trip"):
        assert GRID_ITEMS < _work_items(op, shapes, a) < 2 * GRID_ITEMS
    if name.startswith("sppf_unfused"):
        assert _lib.lib().md_sppf_pool_groups(52, 52, 256) == 0      # the shape on which graphs.SPPF takes this path
    _replay(name, op, shapes, a, 100 + 7 * list(FIXED).index(name))
