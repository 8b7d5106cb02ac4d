"""-m gpu: every decode call one production pass makes -- md_rpn_decode, md_rcnn_scores, md_rcnn_decode_selected, md_mask_select,
md_yolo_decode, md_yolov8_decode, md_heat_peaks, md_centernet_assemble and md_centerpoint_decode -- replayed through the C ABI with
fresh inputs and compared over the WHOLE output with the float64 references of tests/decode_contract.py.

Each model is built from configs/ at its production batch (CenterNet R18 512^2 from graphs.CenterNet, which has no config) and run
once the way production runs it (forward_split: with test_cfg.streams = 2 every call is a half-batch call).  A wrapper around
_lib.call records each decode call's op, shapes and attribute record; the recorded op set must be the model's, so a graph change that
stops calling a kernel fails here.  Every distinct call is then replayed with data from the contract's generators: Gaussian bf16 heads
at a scale that balances each threshold decision, every finite bf16 value as a sigmoid input where the call has that many, exact
class-logit ties, saturated (>= 16) and underflowing (< -87) class logits, NaN in every channel the op must not read, deltas past
max_ratio, boxes across every image edge, first / last anchor and candidate indices, counts of 0, partial and full, heat-map plateaus
across the 8 x 64 tile seams and the border, CenterPoint centres on the range edges and rot (0, 0), and mask rows with score 0, a
negative score, label -1 and label nc.  md_heat_peaks is replayed as recorded (hm NULL) and with hm, so every sigmoid-clipped value is
checked.

Outputs start as a NaN sentinel with sentinel guard zones: elements the call must not write (the other levels' rows of a YOLO output,
the guard zones) keep it bit for bit, every other element loses it.  Continuous outputs must lie within the contract's derived bound
of the float64 value; discrete outputs must match exactly, except for decisions whose float64 inputs lie within the bound of the
boundary, which may go either way -- at most decode_contract.CAP of a case's decisions.  Each case prints its worst err / bound and
its either-outcome share (`pytest -s`)."""
import ctypes
import json
import os

import pytest
import torch

from minddet_amd import _lib
from tests import decode_contract as dc
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x7FA5A5A5       # a float32 NaN bit pattern (as int32) that no output value or label takes
GUARD = 1 << 14             # sentinel elements on each side of every output
CHUNK_ELEMS = 1 << 24       # head elements per float64 reference chunk

DECODE_OPS = ("md_rpn_decode", "md_rcnn_scores", "md_rcnn_decode_selected", "md_mask_select", "md_yolo_decode", "md_yolov8_decode",
              "md_heat_peaks", "md_centernet_assemble", "md_centerpoint_decode")
RCNN = {"md_rpn_decode", "md_rcnn_scores", "md_rcnn_decode_selected"}
# (case, config or None, batch, the decode ops one pass calls)
MODELS = [("faster_rcnn_b120", "configs/faster_rcnn/faster_rcnn_r50_fpn.py", 120, RCNN),
          ("faster_rcnn_b60", "configs/faster_rcnn/faster_rcnn_r50_fpn.py", 60, RCNN),
          ("mask_rcnn_b32", "configs/mask_rcnn/mask_rcnn_r101_fpn.py", 32, RCNN | {"md_mask_select"}),
          ("yolov5s_b32", "configs/yolov5/yolov5s.py", 32, {"md_yolo_decode"}),
          ("yolov8l_b32", "configs/yolov8/yolov8l.py", 32, {"md_yolov8_decode"}),
          ("centerpoint_b4", "configs/centerpoint/centerpoint_pp_nusc.py", 4, {"md_centerpoint_decode"}),
          ("centernet_r18_512_b32", None, 32, {"md_heat_peaks", "md_centernet_assemble"})]


def _fields(s):
    if isinstance(s, ctypes.Array):
        return [_fields(v) for v in s]
    if isinstance(s, ctypes.Structure):
        return {f: _fields(getattr(s, f)) for f, _ in s._fields_}
    if isinstance(s, ctypes._SimpleCData):
        return {"num_classes": s.value}      # md_mask_select's int32 extra
    return s


def _model_input(config, batch):
    """(model, input batch) at the config's production image size: stem layout for the image models, the pseudo-image for CenterPoint"""
    from minddet.models import Config, build_detector
    from minddet_amd import graphs, nn_ops

    if config is None:       # CenterNet takes the [B, H, W, 8] NHWC batch (its .to() builds no fused-stem pack)
        x = torch.zeros((batch, 512, 512, 8), dtype=torch.bfloat16, device=DEV)
        x[..., :3] = torch.randn((batch, 512, 512, 3), device=DEV).to(torch.bfloat16)
        return graphs.CenterNet(depth=18, num_classes=80).to(DEV), x
    else:
        cfg = Config.fromfile(os.path.join(ROOT, config))
        m = build_detector(cfg.model, cfg.train_cfg, cfg.test_cfg).to(DEV)
        if "pseudo_image_hw" in cfg.data:
            h, w = cfg.data["pseudo_image_hw"]
            return m, torch.randn((batch, h, w, cfg.data["pseudo_image_channels"]), device=DEV).to(torch.bfloat16)
        hw = cfg.data["input_hw"]
    h, w = hw
    x4 = torch.zeros((batch, h + nn_ops.STEM_PAD_LO + nn_ops.STEM_PAD_HI, w + nn_ops.STEM_PAD_LO + nn_ops.STEM_PAD_HI, 4),
                     dtype=torch.bfloat16, device=DEV)
    x4[:, nn_ops.STEM_PAD_LO:nn_ops.STEM_PAD_LO + h, nn_ops.STEM_PAD_LO:nn_ops.STEM_PAD_LO + w, :3] = \
        torch.randn((batch, h, w, 3), device=DEV).to(torch.bfloat16)
    return m, x4


def decode_calls(config, batch):
    """the distinct decode calls (op, shapes, attrs dict, extra) of one production pass of the model"""
    m, x = _model_input(config, batch)
    calls, keys, orig = [], set(), _lib.call

    def record(name, tensors, extra=None, stream=None):
        if name in DECODE_OPS:
            shapes = [None if t is None else list(t.shape) for t in tensors]
            attrs = _fields(extra)
            key = json.dumps([name, shapes, attrs])
            if key not in keys:
                keys.add(key)
                cp = None if extra is None else type(extra).from_buffer_copy(extra)
                calls.append((name, shapes, attrs, cp))
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
def _out(shape, dtype):
    """(tensor, flat): an output of `shape` (4-byte dtype) filled with the sentinel, inside a sentinel buffer GUARD elements longer on
    each side"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    return flat[GUARD:GUARD + n].view(dtype).view(shape), flat


def _guards_intact(flat):
    assert bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[-GUARD:] == SENTINEL).all()), "write outside the output tensor"


def _all_written(t, what):
    assert not bool((t.contiguous().view(torch.int32) == SENTINEL).any()), f"{what}: element left unwritten"


class Tally:
    def __init__(self):
        self.worst, self.dec, self.either = 0.0, 0, 0

    def add(self, name, got, x):
        nb, worst, first = dc.check(got, x)
        if nb:
            extra = ""
            if x.val is not None and first is not None:
                extra = f": got {got[first].item()}, want {x.val.v[first].item()} +- {x.val.e[first].item()}"
            elif first is not None:
                extra = f": got {got[first].item()}"
            raise AssertionError(f"{name}: {nb} of {got.numel()} elements wrong; first at {first}{extra}")
        self.worst = max(self.worst, worst)

    def decisions(self, n, e):
        self.dec += n
        self.either += e


def _host(gen, *args):
    """a generator run on the host (index errors in the data set-up raise there instead of trapping on the device), its tensors moved
    to the GPU"""
    ins, plants = gen(*args, "cpu")
    return [None if t is None else t.to(DEV) for t in ins], plants


def _chunks(n, per_image):
    nb = max(1, CHUNK_ELEMS // max(per_image, 1))
    return [(i, min(n, i + nb)) for i in range(0, n, nb)]


def _run(op, shapes, attrs, extra, seed, hm=False):
    t = Tally()
    if op == "md_yolo_decode" or op == "md_yolov8_decode":
        (head,), _ = _host(dc.gen_yolo if op == "md_yolo_decode" else dc.gen_yolov8, shapes[0], attrs, seed)
        (b_, fb), (s_, fs), (l_, fl) = _out(shapes[1], torch.float32), _out(shapes[2], torch.float32), _out(shapes[3], torch.int32)
        _lib.call(op, [head, b_, s_, l_], extra=extra)
        torch.cuda.synchronize()
        B, H, W, _ = head.shape
        per = H * W * (attrs["num_anchors"] if op == "md_yolo_decode" else 1)
        o0, o1 = attrs["out_offset"], attrs["out_offset"] + per
        for f, x in ((fb, b_), (fs, s_), (fl, l_)):
            _guards_intact(f)
            other = torch.cat([x[:, :o0], x[:, o1:]], 1)
            assert bool((other.contiguous().view(torch.int32) == SENTINEL).all()), "write outside the level's rows"
            _all_written(x[:, o0:o1], "rows of the level")
        ref = dc.yolo if op == "md_yolo_decode" else dc.yolov8
        for n0, n1 in _chunks(B, head[0].numel()):
            out, n, e = ref(head[n0:n1], attrs)
            t.decisions(n, e)
            for name, x in (("boxes", b_), ("scores", s_), ("labels", l_)):
                t.add(name, x[n0:n1, o0:o1], out[name])
    elif op == "md_rpn_decode":
        ins, _ = _host(dc.gen_rpn, shapes, attrs, seed)
        (b_, fb), (s_, fs) = _out(shapes[4], torch.float32), _out(shapes[5], torch.float32)
        _lib.call(op, ins + [b_, s_], extra=extra)
        torch.cuda.synchronize()
        head, anchors, idx, cnt = ins
        for f, x in ((fb, b_), (fs, s_)):
            _guards_intact(f)
            _all_written(x, op)
        for n0, n1 in _chunks(head.shape[0], head[0].numel()):
            out, n, e = dc.rpn_decode(head[n0:n1], anchors, idx[n0:n1], cnt[n0:n1], attrs)
            t.decisions(n, e)
            t.add("boxes", b_[n0:n1], out["boxes"])
            t.add("scores", s_[n0:n1], out["scores"])
    elif op == "md_rcnn_scores":
        ins, _ = _host(dc.gen_rcnn_scores, shapes, attrs, seed)
        c_, fc = _out(shapes[2], torch.float32)
        _lib.call(op, ins + [c_], extra=extra)
        torch.cuda.synchronize()
        _guards_intact(fc)
        _all_written(c_, op)
        cls_reg, roi_cnt = ins
        B = roi_cnt.numel()
        post, nc = cls_reg.shape[0] // B, attrs["num_classes"]
        for n0, n1 in _chunks(B, post * cls_reg.shape[1]):
            out, n, e = dc.rcnn_scores(cls_reg[n0 * post:n1 * post], roi_cnt, attrs, rows=(n0, n1, post))
            t.decisions(n, e)
            t.add("cand", c_[n0:n1].reshape(-1, nc), out["cand"])
    elif op == "md_rcnn_decode_selected":
        ins, _ = _host(dc.gen_rcnn_decode, shapes, attrs, seed)
        (b_, fb), (l_, fl) = _out(shapes[4], torch.float32), _out(shapes[5], torch.int32)
        _lib.call(op, ins + [b_, l_], extra=extra)
        torch.cuda.synchronize()
        cls_reg, rois, sel, cnt = ins
        for f, x in ((fb, b_), (fl, l_)):
            _guards_intact(f)
            _all_written(x, op)
        B = sel.shape[0]
        post = cls_reg.shape[0] // B
        for n0, n1 in _chunks(B, post * cls_reg.shape[1]):
            out, n, e = dc.rcnn_decode_selected(cls_reg[n0 * post:n1 * post], rois[n0 * post:n1 * post], sel[n0:n1], cnt[n0:n1],
                                                attrs, post)
            t.decisions(n, e)
            t.add("boxes", b_[n0:n1], out["boxes"])
            t.add("labels", l_[n0:n1], out["labels"])
    elif op == "md_mask_select":
        nc = attrs["num_classes"]
        ins, _ = _host(dc.gen_mask, shapes, nc, seed)
        m_, fm = _out(shapes[2], torch.float32)
        _lib.call(op, ins + [m_], extra=extra)
        torch.cuda.synchronize()
        _guards_intact(fm)
        _all_written(m_, op)
        logits, dets = ins
        for r0, r1 in _chunks(logits.shape[0], logits[0].numel()):
            out, n, e = dc.mask_select(logits[r0:r1], dets[r0:r1], nc)
            t.decisions(n, e)
            t.add("masks", m_[r0:r1], out["masks"])
    elif op == "md_heat_peaks":
        (head,), _ = _host(dc.gen_heat, shapes[0], attrs, seed)
        h_, fh = _out(shapes[1], torch.float32)
        m_, fm = _out(shapes[1], torch.float32) if hm else (None, None)
        _lib.call(op, [head, h_, m_], extra=extra)
        torch.cuda.synchronize()
        _guards_intact(fh)
        _all_written(h_, op)
        if hm:
            _guards_intact(fm)
            _all_written(m_, "hm")
        for n0, n1 in _chunks(head.shape[0], head[0].numel()):
            hmv, heat, _, n, e = dc.heat_peaks(head[n0:n1], attrs)
            t.decisions(n, e)
            t.add("heat", h_[n0:n1], heat)
            if hm:
                ones = torch.ones(hmv.v.shape, dtype=torch.bool, device=DEV)
                t.add("hm", m_[n0:n1], dc.Expect(val=hmv, want_val=ones, want_fill=~ones))
    elif op == "md_centernet_assemble":
        ins, _ = _host(dc.gen_assemble, shapes, seed)
        outs = [_out(shapes[5], torch.float32), _out(shapes[6], torch.int32), _out(shapes[7], torch.int32)]
        _lib.call(op, ins + [o for o, _ in outs], extra=extra)
        torch.cuda.synchronize()
        for o, f in outs:
            _guards_intact(f)
            _all_written(o, op)
        out, n, e = dc.centernet_assemble(*ins)
        for (o, _), name in zip(outs, ("det", "inds", "cls")):
            t.add(name, o, out[name])
    elif op == "md_centerpoint_decode":
        (head,), _ = _host(dc.gen_centerpoint, shapes[0], attrs, seed)
        outs = [_out(shapes[1], torch.float32), _out(shapes[2], torch.int32), _out(shapes[3], torch.float32),
                _out(shapes[4], torch.float32)]
        _lib.call(op, [head] + [o for o, _ in outs], extra=extra)
        torch.cuda.synchronize()
        for o, f in outs:
            _guards_intact(f)
            _all_written(o, op)
        for n0, n1 in _chunks(head.shape[0], head[0].numel()):
            out, n, e = dc.centerpoint(head[n0:n1], attrs)
            t.decisions(n, e)
            for (o, _), name in zip(outs, ("scores", "labels", "boxes", "nms_boxes")):
                t.add(name, o[n0:n1], out[name])
    else:
        raise AssertionError(op)
    return t


@pytest.mark.parametrize("case,config,batch,ops", MODELS, ids=[m[0] for m in MODELS])
def test_decode_production_calls(case, config, batch, ops):
    calls = decode_calls(config, batch)
    assert {c[0] for c in calls} == ops, sorted({c[0] for c in calls})
    for j, (op, shapes, attrs, extra) in enumerate(calls):
        for hm in ((False, True) if op == "md_heat_peaks" else (False,)):
            t = _run(op, shapes, attrs, extra, 9000 + 17 * j + int(hm), hm=hm)
            share = t.either / max(t.dec, 1)
            print(f"{case} {op}{' +hm' if hm else ''} {shapes[0]}: worst err/bound {t.worst:.4f}, either-outcome {t.either} of {t.dec} "
                  f"decisions ({100 * share:.4f} %)")
            assert share <= dc.CAP, f"either-outcome share {share:.2e} above the cap {dc.CAP}"
            torch.cuda.empty_cache()
