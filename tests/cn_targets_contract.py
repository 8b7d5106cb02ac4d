"""The contract of md_cn_assign_targets (include/minddet_hip_cn.h) in vectorised numpy: the target part of COCOHP.preprocess_fn
(centernet/src/dataset.py:343-359) for a batch, every fp32 step in the reference's operation order under NumPy >= 2, radius and Gaussian
in float64.  tests/test_cn_targets_cpu.py shows it equal, bit for bit, to what the reference's own code returned
(tests/golden/cn_target_vectors.npz); tests/test_cn_targets_gpu.py holds the device result to it.  The flip and the affine transform
that det_ops.CenterNetTargets applies in front of the operator are here too (post_affine)."""
import numpy as np

f32 = np.float32
KEYS = ("hm", "ind", "reg_mask", "wh", "reg")


def overlap_of(min_overlap):
    """the float64 value the operator reads from its fp32 attribute: the fp32 value, widened"""
    return float(f32(min_overlap))


def gaussian_radius(height, width, o):
    """image.py:94-114 term by term on integer arrays, in float64"""
    hw, wh = (height + width).astype(np.float64), (width * height).astype(np.float64)
    width, height = width.astype(np.float64), height.astype(np.float64)
    b1 = hw
    c1 = wh * (1 - o) / (1 + o)
    r1 = (b1 + np.sqrt(b1 * b1 - 4 * c1)) / 2
    b2 = 2 * hw
    c2 = (1 - o) * width * height
    r2 = (b2 + np.sqrt(b2 * b2 - 16 * c2)) / 2
    a3 = 4 * o
    b3 = -2 * o * hw
    c3 = (o - 1) * width * height
    r3 = (b3 + np.sqrt(b3 * b3 - 4 * a3 * c3)) / 2
    return np.minimum(np.minimum(r1, r2), r3)


def post_affine(bboxes, trans=None, flip_width=None):
    """original-image boxes [B,G,4] f32 -> the fp32 values the reference holds in `bbox` after the flip (dataset.py:340) and the two
    affine_transform calls (:341-342): trans [B,2,3] float64, flip_width [B] (<= 0: not flipped)"""
    b = np.array(bboxes, f32)
    if flip_width is not None:
        fw = np.asarray(flip_width).astype(f32).reshape(-1, 1)
        x0 = np.where(fw > 0, fw - b[..., 2] - f32(1), b[..., 0])
        x1 = np.where(fw > 0, fw - b[..., 0] - f32(1), b[..., 2])
        b = np.stack([x0, b[..., 1], x1, b[..., 3]], -1).astype(f32)
    if trans is not None:
        t = np.asarray(trans, np.float64)[:, None, None]                 # [B,1,1,2,3]
        p = b.astype(np.float64).reshape(b.shape[0], b.shape[1], 2, 1, 2)
        with np.errstate(invalid="ignore"):
            b = ((t[..., 0] * p[..., 0] + t[..., 1] * p[..., 1]) + t[..., 2]).astype(f32).reshape(b.shape)
    return b


def assign(boxes, classes, *, num_classes, feature_map_size, max_objs, min_overlap=0.7):
    """boxes [B,G,4] f32 (output-map coordinates, before the clip), classes [B,G] -> dict of hm [B,C,H,W] f32, ind [B,M] i32,
    reg_mask [B,M] u8, wh [B,M,2] f32, reg [B,M,2] f32; feature_map_size = (W, H)"""
    boxes, classes = np.asarray(boxes, f32), np.asarray(classes)
    B, G = classes.shape
    C, M, (W, H) = int(num_classes), int(max_objs), feature_map_size
    assert G <= M
    o = overlap_of(min_overlap)
    with np.errstate(invalid="ignore"):
        x0, x1 = np.clip(boxes[..., 0], 0, W - 1), np.clip(boxes[..., 2], 0, W - 1)
        y0, y1 = np.clip(boxes[..., 1], 0, H - 1), np.clip(boxes[..., 3], 0, H - 1)
        h, w = y1 - y0, x1 - x0
        used = (h > 0) & (w > 0) & (classes >= 1) & (classes <= C)
    assert x0.dtype == f32 and h.dtype == f32
    hs, ws = np.where(used, h, f32(1)), np.where(used, w, f32(1))
    radius = np.maximum(0, gaussian_radius(np.ceil(hs).astype(np.int64), np.ceil(ws).astype(np.int64), o).astype(np.int64))
    ctx, cty = np.where(used, (x0 + x1) / f32(2), f32(0)), np.where(used, (y0 + y1) / f32(2), f32(0))
    cx, cy = ctx.astype(np.int32), cty.astype(np.int32)
    out = dict(hm=np.zeros((B, C, H, W), f32), ind=np.zeros((B, M), np.int32), reg_mask=np.zeros((B, M), np.uint8),
               wh=np.zeros((B, M, 2), f32), reg=np.zeros((B, M, 2), f32))
    out["ind"][:, :G] = np.where(used, cy * W + cx, 0)
    out["reg_mask"][:, :G] = used
    out["wh"][:, :G] = np.where(used[..., None], np.stack([w, h], -1), f32(0))
    out["reg"][:, :G] = np.stack([ctx - cx.astype(f32), cty - cy.astype(f32)], -1)
    for b, k in zip(*np.nonzero(used)):
        r, x, y = int(radius[b, k]), int(cx[b, k]), int(cy[b, k])
        sigma = (2 * r + 1) / 6
        ys, xs = np.arange(max(0, y - r), min(H, y + r + 1)), np.arange(max(0, x - r), min(W, x + r + 1))
        dy, dx = (ys - y).astype(np.float64)[:, None], (xs - x).astype(np.float64)[None, :]
        g = np.exp(-(dx * dx + dy * dy) / (2 * sigma * sigma)).astype(f32)
        view = out["hm"][b, classes[b, k] - 1, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
        np.maximum(view, g, out=view)
    return out
